// bfhip_diag.hip -- the data-sized passes of the chains' convergence diagnostics (bayesfast_amd/utils/diagnostics.py: rank-normalised
// split-R-hat, bulk / tail / mean effective sample size, the table of mean, sd and quantiles; Vehtari et al. 2021), on a batch of at
// most DG_B parameters of the (chain, time, dimension) sample tensor:
//
//   bfhip_diag_columns  the batch's columns -> the split layout (2 n_chain, h, DG_B): plain, |x - c_b| or 1[x <= c_b]
//   bfhip_diag_extent   smallest and largest value of every split chain's column (constant parameters, by exact comparison)
//   bfhip_diag_sort     one column of that buffer -> sorted order-preserving keys and the permutation (rocPRIM's radix sort)
//   bfhip_diag_rank     sorted keys and permutation -> z = ndtri((mean rank - 3/8) / (n + 1/4)), scattered back into the buffer
//
// The batch is along the dimension axis because the sampler stores samples time-major: DG_B doubles are 128 contiguous bytes of
// every sample row, and 16 lanes read them in one request.  The series buffer is always DG_B wide (unused columns are zero), so
// the chain moments and lag sums on it (bfhip_acor_moments, bfhip_acor_lag_sums with n_d = DG_B) run in one shape and one
// summation order whichever batch a parameter falls in.  Everything here is elementwise, a minimum / maximum, a stable sort or a search: no
// floating-point reduction, bitwise repeatable.  64-bit offsets throughout.
#include "bfhip_block.h"
#include "bfhip_ndtri.h"

#define DG_B BFHIP_DIAG_BATCH
static_assert(DG_B == 16 && 256 / DG_B == BF_SLICES, "the column index is taken with a mask; bf_slice_fold's layout");

// ---- columns: element e = (piece j, step i, column b), b fastest ------------------------------------------------------------------
// A chain is cut into SPLIT pieces of h steps: piece j = SPLIT chain + half starts at row half h of its chain (SPLIT 1: the whole
// chain).  A row of weight 0 (w given) becomes NaN: not part of the weighted sample, it sorts last, whatever it holds.
template <typename T, int SPLIT>
__global__ __launch_bounds__(256) void bf_columns_kernel(long n_el, long h, long ldw, long ldr, const T *__restrict__ x, int nb, int mode,
                                                        const double *__restrict__ c, const double *__restrict__ w,
                                                        double *__restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_el) return;
    const int b = (int)(e & (DG_B - 1));
    const long row = e / DG_B;           // j h + i
    const long j = row / h, i = row - j * h;
    double v = 0.;
    if (b < nb) {
        v = (double)x[(j / SPLIT) * ldw + ((j % SPLIT) * h + i) * ldr + b];
        if (mode == BFHIP_DIAG_FOLD) v = fabs(v - c[b]);
        else if (mode == BFHIP_DIAG_BELOW) v = v <= c[b] ? 1. : 0.;   // (a NaN compares false; such a column is reported as NaN)
        if (w && w[row] == 0.) v = __builtin_nan("");
    }
    out[e] = v;
}

template <typename T>
static void bf_columns_typed(hipStream_t st, int split, long n_el, long h, long ldw, long ldr, const T *x, int nb, int mode,
                             const double *c, const double *w, double *out) {
    const dim3 grid((unsigned)((n_el + 255) / 256));
    if (split == 2) hipLaunchKernelGGL((bf_columns_kernel<T, 2>), grid, dim3(256), 0, st, n_el, h, ldw, ldr, x, nb, mode, c, w, out);
    else hipLaunchKernelGGL((bf_columns_kernel<T, 1>), grid, dim3(256), 0, st, n_el, h, ldw, ldr, x, nb, mode, c, w, out);
}

int bf_columns_launch(bfhip_ctx *ctx, int split, long n_el, long h, long ldw, long ldr, const void *x, int is_f32, long off, int nb,
                      int mode, const double *c, const double *w, double *out) {
    if (is_f32) bf_columns_typed(ctx->stream, split, n_el, h, ldw, ldr, (const float *)x + off, nb, mode, c, w, out);
    else bf_columns_typed(ctx->stream, split, n_el, h, ldw, ldr, (const double *)x + off, nb, mode, c, w, out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int bfhip_diag_columns(bfhip_ctx *ctx, int n_chain, long h, long ldw, long ldr, const void *x, int is_f32, long since,
                                  int k0, int nb, int mode, const double *c, double *out) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n_chain < 1 || h < 1 || !x || !out || since < 0 || k0 < 0 || nb < 1 || nb > DG_B || ldr < (long)k0 + nb ||
        (n_chain > 1 && ldw < 1) || mode < BFHIP_DIAG_PLAIN || mode > BFHIP_DIAG_BELOW || (mode != BFHIP_DIAG_PLAIN && !c))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_diag_columns: invalid argument");
    const long n_el = 2L * n_chain * h * DG_B, nblk = (n_el + 255) / 256;
    if (2L * n_chain * h > 0x7fffffffL || nblk > 0x7fffffffL)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_diag_columns: more than 2^31-1 values per column");
    return bf_columns_launch(ctx, 2, n_el, h, ldw, ldr, x, is_f32, since * ldr + k0, nb, mode, c, nullptr, out);
}

// ---- extent: one workgroup per split chain, 16 columns x 16 time slices; min and max are exact in any order ---------------------------
__global__ __launch_bounds__(256) void bf_diag_extent_kernel(long h, const double *__restrict__ series, double *__restrict__ lo,
                                                            double *__restrict__ hi) {
    __shared__ double mn[256], mx[256];
    const int b = threadIdx.x & (DG_B - 1), sl = threadIdx.x / DG_B;
    const double *s = series + (long)blockIdx.x * h * DG_B + b;
    double a = __builtin_inf(), e = -__builtin_inf();
    for (long i = sl; i < h; i += 256 / DG_B) {
        const double v = s[i * DG_B];
        a = fmin(a, v);   // (fmin / fmax return the other operand for a NaN)
        e = fmax(e, v);
    }
    mn[threadIdx.x] = a;
    mx[threadIdx.x] = e;
    __syncthreads();
    if (sl == 0) {
        a = bf_slice_fold(a, 1, mn, b, BfMin());
        e = bf_slice_fold(e, 1, mx, b, BfMax());
        lo[(long)blockIdx.x * DG_B + b] = a;
        hi[(long)blockIdx.x * DG_B + b] = e;
    }
}

extern "C" int bfhip_diag_extent(bfhip_ctx *ctx, int n_series, long h, const double *series, double *lo, double *hi) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n_series < 1 || h < 1 || !series || !lo || !hi)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_diag_extent: invalid argument");
    hipLaunchKernelGGL(bf_diag_extent_kernel, dim3((unsigned)n_series), dim3(256), 0, ctx->stream, h, series, lo, hi);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- sort of one column ----------------------------------------------------------------------------------------------------------
extern "C" int bfhip_diag_sort(bfhip_ctx *ctx, long n, const double *series, int b, uint64_t *keys_sorted, uint32_t *order) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || !series || b < 0 || b >= DG_B || !keys_sorted || !order)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_diag_sort: invalid argument");
    if (n > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_diag_sort: more than 2^31-1 elements");
    return bf_sort_column(ctx, n, series, DG_B, b, keys_sorted, order);
}

// ---- ranks with ties -> normal scores ----------------------------------------------------------------------------------------------
// Sorted position p holds rank p + 1 unless a neighbour has the same key; then the tie run [lo, hi) is found by bisection (as
// bf_count_keys_kernel) and its members share the mean of the ranks lo + 1 .. hi, (lo + 1 + hi) / 2: a half-integer, exact.
__global__ __launch_bounds__(256) void bf_diag_rank_kernel(long n, const uint64_t *__restrict__ ks, const uint32_t *__restrict__ order,
                                                          int b, double *__restrict__ z) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint64_t k = ks[p];
    long lo = p, hi = p + 1;
    if (p > 0 && ks[p - 1] == k) {
        long a = 0, e = p;          // first position whose key is not below k
        while (a < e) {
            const long mid = (a + e) >> 1;
            if (ks[mid] < k) a = mid + 1;
            else e = mid;
        }
        lo = a;
    }
    if (p + 1 < n && ks[p + 1] == k) {
        long a = p + 1, e = n;      // first position whose key is above k
        while (a < e) {
            const long mid = (a + e) >> 1;
            if (ks[mid] <= k) a = mid + 1;
            else e = mid;
        }
        hi = a;
    }
    const double r = 0.5 * (double)(lo + 1 + hi);
    z[(long)order[p] * DG_B + b] = bf_ndtri((r - 0.375) / ((double)n + 0.25));   // (order[p] < n: a permutation of 0 .. n - 1)
}

extern "C" int bfhip_diag_rank(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, const uint32_t *order, int b, double *z) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !keys_sorted || !order || b < 0 || b >= DG_B || !z)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_diag_rank: invalid argument");
    hipLaunchKernelGGL(bf_diag_rank_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, keys_sorted, order, b, z);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
