// bfhip_marg.hip -- marginal posterior histograms and credible levels of weighted draws (bayesfast_amd/utils/marginals.py has the
// definitions), where sample() left the chains:
//
//   bfhip_marg_quantise  normalised weights w' in [0, 1] -> fixed-point weights q = floor(w' 2^k), uint64; a count of unusable weights
//   bfhip_marg_extent    a (n, MG_B) series buffer -> per column the smallest and largest finite value among the rows with q > 0
//   bfhip_marg_hist1d    series buffer, q, per-column lo / hi / inv -> hist (MG_B, n_bins) and outside (MG_B, 3), ADDED to the buffers
//   bfhip_marg_index     series buffer -> one uint8 bin index per value (255: not in range) into columns col0 .. of idx (n, ld)
//   bfhip_marg_hist2d    idx, a list of column pairs, q -> hist (n_pair, n_bins, n_bins), ADDED to the buffer: the hot path
//   bfhip_marg_levels    a workgroup per histogram: its sum and, per probability, the largest bin value v with sum(bins >= v) >= p sum
//
// Everything that is accumulated is a 64-bit integer: sums of integers do not depend on their order, so LDS and global atomics
// may be used freely and the results are still bitwise repeatable, whatever the launch shape, the tiling or the sharding of the
// rows.  The only floating-point arithmetic is elementwise: the scaling of a weight by a power of two, and the bin of a value,
// floor((x - lo) inv): a subtraction, then a multiplication (nothing to contract; the file is built with -ffp-contract=off all
// the same).  64-bit offsets throughout, n <= 2^31 - 1.
//
// The pair kernel: a workgroup of 1024 threads owns a chunk of rows and a group of P pairs, whose private histograms it keeps in
// LDS as uint64 (P n_bins^2 8 bytes: 4 pairs at 64 x 64, one at 128 x 128).  It walks its chunk in tiles of 16384 index bytes
// (16384 / ld rows), which it copies into LDS once, one 16-byte vector per thread -- the next tile's vector is loaded before
// the current tile is worked on -- and every (row, pair) of the tile is one thread's two byte reads from that copy and one
// 64-bit LDS atomic add.  The tile rows are padded by one word, so 32 consecutive rows read 32 different banks.  At the end the
// non-zero bins are added to the global histograms by 64-bit global atomics.  The pair group is the fastest grid dimension:
// the workgroups resident together work on the same rows, which they find in the L2.
#include "bfhip_block.h"

#define MG_T 256                    // threads per workgroup of everything but the pair kernel
#define MG_B BFHIP_DIAG_BATCH
#define MG_ROWS (MG_T / MG_B)       // row slices of a workgroup of the column passes
#define MG_MAXB 1024                // workgroups of the extent pass (they stride over the rows beyond)
#define MG_H1_ROWS 4096             // rows per workgroup of the 1-D histogram before the grid stops growing ...
#define MG_H1_MAXB 512              // ... at this many workgroups (each flushes up to MG_B n_bins bins)
#define MG2_T 1024                  // threads of the pair kernel
#define MG2_TILE 16384              // index bytes per row tile: one 16-byte vector per thread
#define MG2_PMAX 16                 // pairs per workgroup at most
#define MG2_LDS 163840              // LDS of a CU
#define MG2_MAXCHUNK 1024           // row chunks at most
static_assert(MG_B == 16 && MG_ROWS == BF_SLICES, "the column index is taken with a mask; bf_slice_fold's layout");
static_assert(MG2_TILE == 16 * MG2_T, "one vector per thread and tile");
static_assert(BFHIP_MARG_EXTENT_WORK >= 2 * MG_MAXB * MG_B, "bfhip_marg_extent keeps two partial arrays");

typedef unsigned long long mg_u64;

// ---- weights ------------------------------------------------------------------------------------------------------------------------
// q = floor(w' 2^k): w' 2^k is exact (a power of two), <= 2^62.  A weight that is negative, NaN or above 1 counts in *flag, q = 0.
__global__ __launch_bounds__(MG_T) void mg_quantise_kernel(long n, const double *__restrict__ wp, int k, uint64_t *__restrict__ q,
                                                          mg_u64 *__restrict__ flag) {
    __shared__ unsigned sbad;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    const double scale = (double)(1ull << k);
    unsigned bad = 0;
    for (long i = (long)blockIdx.x * MG_T + threadIdx.x; i < n; i += (long)gridDim.x * MG_T) {
        uint64_t v = 1;
        if (wp) {
            const double w = wp[i];
            if (!(w >= 0.) || w > 1.) {
                ++bad;
                v = 0;
            } else v = (uint64_t)floor(w * scale);
        }
        q[i] = v;
    }
    if (bad) atomicAdd(&sbad, bad);
    __syncthreads();
    if (threadIdx.x == 0 && sbad) atomicAdd(flag, (mg_u64)sbad);
}

extern "C" int bfhip_marg_quantise(bfhip_ctx *ctx, long n, const double *wp, int k, uint64_t *q, uint64_t *flag) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || k < 0 || k > 62 || !q || !flag)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_marg_quantise: invalid argument");
    const long g = (n + MG_T - 1) / MG_T;
    hipLaunchKernelGGL(mg_quantise_kernel, dim3((unsigned)(g > MG_MAXB ? MG_MAXB : g)), dim3(MG_T), 0, ctx->stream, n, wp, k, q,
                       (mg_u64 *)flag);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- extent: thread (slice sl, column b) walks rows sl, sl + 16 G, ...; min and max are exact in any order ----------------------------
__global__ __launch_bounds__(MG_T) void mg_extent_kernel(long n, const double *__restrict__ series, const uint64_t *__restrict__ q,
                                                        double *__restrict__ part) {
    __shared__ double mn[MG_T], mx[MG_T];
    const int b = threadIdx.x & (MG_B - 1), sl = threadIdx.x / MG_B;
    double a = __builtin_inf(), e = -__builtin_inf();
    for (long r = (long)blockIdx.x * MG_ROWS + sl; r < n; r += (long)gridDim.x * MG_ROWS) {
        if (q && q[r] == 0) continue;   // not part of the sample, whatever it holds
        const double v = series[r * MG_B + b];
        if (fabs(v) < __builtin_inf()) {
            a = fmin(a, v);
            e = fmax(e, v);
        }
    }
    mn[threadIdx.x] = a;
    mx[threadIdx.x] = e;
    __syncthreads();
    if (sl == 0) {
        part[(long)blockIdx.x * MG_B + b] = bf_slice_fold(a, 1, mn, b, BfMin());
        part[((long)MG_MAXB + blockIdx.x) * MG_B + b] = bf_slice_fold(e, 1, mx, b, BfMax());
    }
}

__global__ __launch_bounds__(MG_T) void mg_extent_final_kernel(int nb, const double *__restrict__ part, double *__restrict__ lo,
                                                              double *__restrict__ hi) {
    __shared__ double mn[MG_T], mx[MG_T];
    const int b = threadIdx.x & (MG_B - 1), sl = threadIdx.x / MG_B;
    double a = __builtin_inf(), e = -__builtin_inf();
    for (int g = sl; g < nb; g += MG_ROWS) {
        a = fmin(a, part[(long)g * MG_B + b]);
        e = fmax(e, part[((long)MG_MAXB + g) * MG_B + b]);
    }
    mn[threadIdx.x] = a;
    mx[threadIdx.x] = e;
    __syncthreads();
    if (sl == 0) {
        lo[b] = bf_slice_fold(a, 1, mn, b, BfMin());
        hi[b] = bf_slice_fold(e, 1, mx, b, BfMax());
    }
}

extern "C" int bfhip_marg_extent(bfhip_ctx *ctx, long n, const double *series, const uint64_t *q, double *lo, double *hi, double *work) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !series || !lo || !hi || !work)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_marg_extent: invalid argument");
    const long g = (n + MG_ROWS - 1) / MG_ROWS;
    const int nb = (int)(g > MG_MAXB ? MG_MAXB : g);
    hipLaunchKernelGGL(mg_extent_kernel, dim3(nb), dim3(MG_T), 0, ctx->stream, n, series, q, work);
    hipLaunchKernelGGL(mg_extent_final_kernel, dim3(1), dim3(MG_T), 0, ctx->stream, nb, work, lo, hi);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- the bin of a value: 0 .. B - 1, or B below, B + 1 above, B + 2 not finite (or edges that are NaN) -----------------------------
__device__ inline int mg_slot(double v, double lo, double hi, double inv, int B) {
    if (!(fabs(v) < __builtin_inf())) return B + 2;
    if (v < lo) return B;
    if (v > hi) return B + 1;
    if (!(lo <= v && v <= hi)) return B + 2;
    const double t = floor((v - lo) * inv);           // 0 <= t, and t <= B up to rounding
    return t < (double)(B - 1) ? (int)t : B - 1;
}

// ---- 1-D histograms: private copies in LDS, 64-bit integer atomics there, the non-zero bins added to the global ones --------------
__global__ __launch_bounds__(MG_T) void mg_hist1d_kernel(long n, const double *__restrict__ series, const uint64_t *__restrict__ q,
                                                        const double *__restrict__ lo, const double *__restrict__ hi,
                                                        const double *__restrict__ inv, int nb, int B, mg_u64 *__restrict__ hist,
                                                        mg_u64 *__restrict__ outside) {
    extern __shared__ __attribute__((aligned(16))) mg_u64 mg_lh1[];   // (MG_B, B) bins, then (MG_B, 3)
    const int n_bin = MG_B * B, tot = n_bin + MG_B * 3;
    for (int e = threadIdx.x; e < tot; e += MG_T) mg_lh1[e] = 0;
    __syncthreads();
    const int b = threadIdx.x & (MG_B - 1), sl = threadIdx.x / MG_B;
    if (b < nb) {
        const double l = lo[b], h = hi[b], iv = inv[b];
        for (long r = (long)blockIdx.x * MG_ROWS + sl; r < n; r += (long)gridDim.x * MG_ROWS) {
            const mg_u64 qv = q ? q[r] : 1;
            if (qv == 0) continue;
            const int s = mg_slot(series[r * MG_B + b], l, h, iv, B);
            atomicAdd(s < B ? &mg_lh1[b * B + s] : &mg_lh1[n_bin + b * 3 + (s - B)], qv);
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < tot; e += MG_T) {
        const mg_u64 v = mg_lh1[e];
        if (v) atomicAdd(e < n_bin ? &hist[e] : &outside[e - n_bin], v);
    }
}

extern "C" int bfhip_marg_hist1d(bfhip_ctx *ctx, long n, const double *series, const uint64_t *q, const double *lo, const double *hi,
                                 const double *inv, int nb, int n_bins, uint64_t *hist, uint64_t *outside) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !series || !lo || !hi || !inv || nb < 1 || nb > MG_B || n_bins < 1 ||
        n_bins > BFHIP_MARG_MAX_BINS || !hist || !outside)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_marg_hist1d: invalid argument");
    const size_t lds = (size_t)(MG_B * n_bins + MG_B * 3) * sizeof(mg_u64);
    if (int rc = bf_set_lds(mg_hist1d_kernel, lds)) return rc;
    const long g = (n + MG_H1_ROWS - 1) / MG_H1_ROWS;
    hipLaunchKernelGGL(mg_hist1d_kernel, dim3((unsigned)(g > MG_H1_MAXB ? MG_H1_MAXB : g)), dim3(MG_T), lds, ctx->stream, n, series, q,
                       lo, hi, inv, nb, n_bins, (mg_u64 *)hist, (mg_u64 *)outside);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- bin indices: element e = (row, column b), b fastest ------------------------------------------------------------------------------
__global__ __launch_bounds__(MG_T) void mg_index_kernel(long n_el, const double *__restrict__ series, const double *__restrict__ lo,
                                                       const double *__restrict__ hi, const double *__restrict__ inv, int nb, int B,
                                                       uint8_t *__restrict__ idx, long ld, int col0) {
    const long e = (long)blockIdx.x * MG_T + threadIdx.x;
    if (e >= n_el) return;
    const int b = (int)(e & (MG_B - 1));
    if (b >= nb) return;
    const int s = mg_slot(series[e], lo[b], hi[b], inv[b], B);
    idx[(e / MG_B) * ld + col0 + b] = (uint8_t)(s < B ? s : 255);
}

extern "C" int bfhip_marg_index(bfhip_ctx *ctx, long n, const double *series, const double *lo, const double *hi, const double *inv,
                                int nb, int n_bins, uint8_t *idx, long ld, int col0) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !series || !lo || !hi || !inv || nb < 1 || nb > MG_B || n_bins < 1 ||
        n_bins > BFHIP_MARG_MAX_BINS2D || !idx || col0 < 0 || ld < (long)col0 + nb)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_marg_index: invalid argument");
    const long n_el = n * MG_B;
    hipLaunchKernelGGL(mg_index_kernel, dim3((unsigned)((n_el + MG_T - 1) / MG_T)), dim3(MG_T), 0, ctx->stream, n_el, series, lo, hi, inv,
                       nb, n_bins, idx, ld, col0);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- 2-D histograms ------------------------------------------------------------------------------------------------------------------
// grid (pair groups, row chunks).  LDS: P B^2 uint64 bins | the tile, R rows of ld / 4 + 1 words | 2 P columns.
__device__ inline uint4 mg2_load(const uint4 *__restrict__ src, long base, long r1, int ld) {
    const long row = base + (long)(threadIdx.x * 16) / ld;
    if (row < r1) return src[(base * ld) / 16 + threadIdx.x];   // (bytes of a row below n: inside the matrix)
    return make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
}

__global__ __launch_bounds__(MG2_T) void mg_hist2d_kernel(long n, const uint8_t *__restrict__ idx, int ld, const int32_t *__restrict__ pairs,
                                                         long n_pair, const uint64_t *__restrict__ q, int B, int P, long chunk_rows,
                                                         mg_u64 *__restrict__ hist) {
    extern __shared__ __attribute__((aligned(16))) mg_u64 mg_lds2[];
    const int R = MG2_TILE / ld, ldw = ld / 4 + 1, t = threadIdx.x;
    const int r_shift = 31 - __builtin_clz(R);    // R is a power of two
    mg_u64 *lh = mg_lds2;
    uint32_t *tile = (uint32_t *)(lh + (size_t)P * B * B);
    int *cols = (int *)(tile + R * ldw);
    const long p0 = (long)blockIdx.x * P;
    const int np = (int)(n_pair - p0 < (long)P ? n_pair - p0 : (long)P), n_bin = np * B * B;
    for (int e = t; e < n_bin; e += MG2_T) lh[e] = 0;
    if (t < 2 * np) {
        const int c = pairs[2 * p0 + t];
        cols[t] = (c >= 0 && c < ld) ? c : -1;     // a pair with a column outside the matrix adds nothing
    }
    const long r0 = (long)blockIdx.y * chunk_rows, r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
    const uint4 *src = (const uint4 *)idx;
    const int t_row = (t * 16) / ld, t_word = ((t * 16) % ld) / 4;
    uint4 nxt = mg2_load(src, r0, r1, ld);
    for (long base = r0; base < r1; base += R) {
        uint32_t *dst = tile + t_row * ldw + t_word;
        dst[0] = nxt.x;
        dst[1] = nxt.y;
        dst[2] = nxt.z;
        dst[3] = nxt.w;
        __syncthreads();
        if (base + R < r1) nxt = mg2_load(src, base + R, r1, ld);
        for (int e = t; e < R * np; e += MG2_T) {
            const int rr = e & (R - 1), p = e >> r_shift;
            const long r = base + rr;
            if (r >= r1) continue;
            const mg_u64 qv = q ? q[r] : 1;
            const int ci = cols[2 * p], cj = cols[2 * p + 1];
            if (qv == 0 || ci < 0 || cj < 0) continue;
            const uint32_t a = (tile[rr * ldw + (ci >> 2)] >> ((ci & 3) * 8)) & 0xffu;
            const uint32_t c = (tile[rr * ldw + (cj >> 2)] >> ((cj & 3) * 8)) & 0xffu;
            if (a < (uint32_t)B && c < (uint32_t)B) atomicAdd(&lh[((size_t)p * B + a) * B + c], qv);
        }
        __syncthreads();
    }
    __syncthreads();   // (a chunk without rows: the zeroes above)
    for (int e = t; e < n_bin; e += MG2_T) {
        const mg_u64 v = lh[e];
        if (v) atomicAdd(&hist[p0 * B * B + e], v);
    }
}

// the launch shape: rows of a tile, pairs per workgroup, LDS bytes, rows per chunk
static inline void mg2_shape(long n, int ld, long n_pair, int B, int *P, size_t *lds, long *chunk_rows) {
    const int R = MG2_TILE / ld, ldw = ld / 4 + 1;
    const size_t fixed = (size_t)R * ldw * 4 + 2 * MG2_PMAX * sizeof(int), per_pair = (size_t)B * B * sizeof(mg_u64);
    long p = (long)((MG2_LDS - fixed) / per_pair);
    if (p > MG2_PMAX) p = MG2_PMAX;
    if (p > n_pair) p = n_pair;
    *P = (int)p;
    *lds = (size_t)p * per_pair + fixed;
    long c = 8L * B * B;                                  // a flush of B^2 bins per pair is worth at least 8 B^2 rows
    if ((n + MG2_MAXCHUNK - 1) / MG2_MAXCHUNK > c) c = (n + MG2_MAXCHUNK - 1) / MG2_MAXCHUNK;
    *chunk_rows = (c + R - 1) / R * R;
}

extern "C" int bfhip_marg_hist2d(bfhip_ctx *ctx, long n, const uint8_t *idx, long ld, const int32_t *pairs, long n_pair, const uint64_t *q,
                                 int n_bins, uint64_t *hist) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !idx || !pairs || n_pair < 1 || n_bins < 1 || n_bins > BFHIP_MARG_MAX_BINS2D || !hist ||
        ((uintptr_t)idx & 15))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_marg_hist2d: invalid argument");
    if (ld < 16 || ld > BFHIP_MARG_MAX_LD || (ld & (ld - 1)))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_marg_hist2d: ld = %ld is not a power of two from 16 to %d", ld, BFHIP_MARG_MAX_LD);
    if ((double)n_pair * n_bins * n_bins > 2147483647.)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_marg_hist2d: more than 2^31-1 bins");
    int P;
    size_t lds;
    long chunk_rows;
    mg2_shape(n, (int)ld, n_pair, n_bins, &P, &lds, &chunk_rows);
    if (int rc = bf_set_lds(mg_hist2d_kernel, lds)) return rc;
    const dim3 grid((unsigned)((n_pair + P - 1) / P), (unsigned)((n + chunk_rows - 1) / chunk_rows));
    hipLaunchKernelGGL(mg_hist2d_kernel, grid, dim3(MG2_T), lds, ctx->stream, n, idx, (int)ld, pairs, n_pair, q, n_bins, P, chunk_rows,
                       (mg_u64 *)hist);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- levels ---------------------------------------------------------------------------------------------------------------------------
// C(v) = sum of the bins >= v does not grow with v, and C(0) = S passes the test, so the largest v that passes is built bit by
// bit from the top: at most 64 rounds of a count over the histogram (it stays in the L2) and an integer block sum.  That v is a
// bin value: between two bin values C does not change.  A descending sort in LDS with a scan would be exact too, but takes
// log2(m)(log2(m) + 1) / 2 = 105 compare-exchange sweeps of 128 KB of LDS at m = 16384, against 64 read sweeps here.
template <bool MAX>
__device__ inline mg_u64 mg_block_u64(mg_u64 v, mg_u64 *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = MG_T / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const mg_u64 a = red[threadIdx.x], b = red[threadIdx.x + o];
            red[threadIdx.x] = MAX ? (a > b ? a : b) : a + b;
        }
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(MG_T) void mg_levels_kernel(long m, const mg_u64 *__restrict__ hist, int n_p, const double *__restrict__ probs,
                                                        mg_u64 *__restrict__ levels, mg_u64 *__restrict__ total) {
    __shared__ mg_u64 red[MG_T];
    const mg_u64 *h = hist + (long)blockIdx.x * m;
    mg_u64 s = 0, mx = 0;
    for (long i = threadIdx.x; i < m; i += MG_T) {
        const mg_u64 v = h[i];
        s += v;
        mx = v > mx ? v : mx;
    }
    s = mg_block_u64<false>(s, red);
    mx = mg_block_u64<true>(mx, red);
    if (threadIdx.x == 0) total[blockIdx.x] = s;
    for (int ip = 0; ip < n_p; ++ip) {
        mg_u64 lvl = 0;
        if (s > 0) {      // (then mx > 0)
            const double need = probs[ip] * (double)s;
            for (int bit = 63 - __builtin_clzll(mx); bit >= 0; --bit) {
                const mg_u64 cand = lvl | (1ull << bit);
                mg_u64 c = 0;
                for (long i = threadIdx.x; i < m; i += MG_T) {
                    const mg_u64 v = h[i];
                    if (v >= cand) c += v;
                }
                c = mg_block_u64<false>(c, red);
                if ((double)c >= need) lvl = cand;
            }
        }
        if (threadIdx.x == 0) levels[(long)blockIdx.x * n_p + ip] = lvl;
    }
}

extern "C" int bfhip_marg_levels(bfhip_ctx *ctx, long n_hist, long m, const uint64_t *hist, int n_p, const double *probs, uint64_t *levels,
                                 uint64_t *total) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n_hist < 1 || n_hist > 0x7fffffffL || m < 1 || m > BFHIP_MARG_MAX_BINS2D * BFHIP_MARG_MAX_BINS2D || !hist || n_p < 1 ||
        !probs || !levels || !total)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_marg_levels: invalid argument");
    hipLaunchKernelGGL(mg_levels_kernel, dim3((unsigned)n_hist), dim3(MG_T), 0, ctx->stream, m, (const mg_u64 *)hist, n_p, probs,
                       (mg_u64 *)levels, (mg_u64 *)total);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
