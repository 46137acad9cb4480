// bfhip_refit.hip -- refit glue on the device: the rank selection behind SystematicResampler
// (utils/misc.py:61-108: `np.argsort(a)[i_all]`), its sharded form (counts of keys below a query, for the exact
// distributed selection of bayesfast_amd/core/refit.py), and the truncated importance weights of PostStep
// (core/recipe.py:1289-1296).  HBM-bound integer / elementwise work: one pass per kernel, the sort is rocPRIM's
// device radix sort (a plain library primitive, like rocBLAS for a plain GEMM).
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include "bfhip_block.h"

// keys[i] = the order key of a[i * stride + col]; idx[i] = i where a permutation is wanted
template <typename Index>
__global__ __launch_bounds__(256) void bf_keys_kernel(long n, const double *__restrict__ a, long stride, int col,
                                                     uint64_t *__restrict__ keys, Index *__restrict__ idx) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        keys[i] = bf_order_key(a[i * stride + col]);
        if (idx) idx[i] = (Index)i;
    }
}

template <typename Index>
int bf_sort_column(bfhip_ctx *ctx, long n, const double *a, long stride, int col, uint64_t *keys_sorted, Index *order) {
    size_t tmp = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const Index *)nullptr,
                                             (Index *)nullptr, (size_t)n, 0, 64, ctx->stream);
    if (e != hipSuccess) return bf_set_error(BFHIP_ERR_HIP, "rocprim::radix_sort_pairs (size query): %s", hipGetErrorString(e));
    // unsorted keys and indices live in the context's workspace, next to rocPRIM's temporary storage
    const size_t kb = ((size_t)n * 8 + 255) / 256 * 256, ib = ((size_t)n * sizeof(Index) + 255) / 256 * 256;
    if (int rc = bf_grow(ctx, &ctx->scratch, &ctx->scratch_bytes, kb + ib + tmp)) return rc;
    uint64_t *k0 = (uint64_t *)ctx->scratch;
    Index *i0 = (Index *)((char *)ctx->scratch + kb);
    void *t = (char *)ctx->scratch + kb + ib;
    hipLaunchKernelGGL(bf_keys_kernel<Index>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, a, stride, col, k0, i0);
    BF_HIP_CHECK(hipGetLastError());
    e = rocprim::radix_sort_pairs(t, tmp, k0, keys_sorted, i0, order, (size_t)n, 0, 64, ctx->stream);  // stable
    if (e != hipSuccess) return bf_set_error(BFHIP_ERR_HIP, "rocprim::radix_sort_pairs: %s", hipGetErrorString(e));
    return 0;
}
template int bf_sort_column<int64_t>(bfhip_ctx *, long, const double *, long, int, uint64_t *, int64_t *);
template int bf_sort_column<uint32_t>(bfhip_ctx *, long, const double *, long, int, uint64_t *, uint32_t *);

extern "C" int bfhip_sort_keys(bfhip_ctx *ctx, long n, const double *a, uint64_t *keys_sorted, int64_t *order) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 0 || (n > 0 && (!a || !keys_sorted || !order)))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_sort_keys: invalid argument");
    if (n == 0) return 0;
    if (n > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_sort_keys: more than 2^31-1 elements");
    return bf_sort_column(ctx, n, a, 1, 0, keys_sorted, order);
}

extern "C" int bfhip_order_keys(bfhip_ctx *ctx, long n, const double *a, uint64_t *keys) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 0 || (n > 0 && (!a || !keys))) return bf_set_error(BFHIP_ERR_ARG, "bfhip_order_keys: invalid argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(bf_keys_kernel<int64_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, a, 1L, 0, keys,
                       (int64_t *)nullptr);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// counts[i] = #{ k : keys_sorted[k] < q[i] }  (upper = 0)  or  #{ k : keys_sorted[k] <= q[i] }  (upper = 1)
__global__ void bf_count_keys_kernel(long n, const uint64_t *__restrict__ ks, long nq, const uint64_t *__restrict__ q, int upper,
                                     int64_t *__restrict__ counts) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const uint64_t v = q[i];
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        const uint64_t k = ks[mid];
        if (upper ? (k <= v) : (k < v)) lo = mid + 1;
        else hi = mid;
    }
    counts[i] = lo;
}

extern "C" int bfhip_count_keys(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, long nq, const uint64_t *q, int upper,
                                int64_t *counts) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 0 || nq < 0 || (n > 0 && !keys_sorted) || (nq > 0 && (!q || !counts)))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_count_keys: invalid argument");
    if (nq == 0) return 0;
    hipLaunchKernelGGL(bf_count_keys_kernel, dim3((unsigned)((nq + 127) / 128)), dim3(128), 0, ctx->stream, n, keys_sorted, nq, q,
                       upper, counts);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- truncated importance weights: w = exp(logp - logq), w_trunc = clip(w, 0, mean(w) n^k) ---------------------
__global__ void bf_iw_exp_kernel(long n, const double *__restrict__ logp, const double *__restrict__ logq, double *__restrict__ w,
                                 double *__restrict__ partial) {
    __shared__ double red[256];
    double s = 0.;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double v = exp(logp[i] - logq[i]);
        w[i] = v;
        s += v;
    }
    s = bf_block_reduce<256, true>(s, red, BfSum());
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void bf_iw_clip_kernel(long n, const double *__restrict__ w, const double *__restrict__ partial, int n_part, double k_trunc,
                                  double *__restrict__ wt) {
    // every block adds the partial sums in the same order: one deterministic mean
    double tot = 0.;
    for (int i = 0; i < n_part; ++i) tot += partial[i];
    const double cap = (tot / (double)n) * pow((double)n, k_trunc);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const double v = w[i];
        // np.clip(w, 0, cap) propagates NaN from either side: a NaN weight stays NaN, and a NaN cap (some weight was NaN)
        // makes every truncated weight NaN
        wt[i] = k_trunc < 0. ? v : (cap != cap ? cap : (v < 0. ? 0. : (v > cap ? cap : v)));
    }
}

extern "C" int bfhip_importance_weights(bfhip_ctx *ctx, long n, const double *logp, const double *logq, double k_trunc, double *w,
                                        double *w_trunc) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 0 || (n > 0 && (!logp || !logq || !w || !w_trunc)))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_importance_weights: invalid argument");
    if (n == 0) return 0;
    const int nb = (int)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);
    if (int rc = bf_grow(ctx, &ctx->scratch, &ctx->scratch_bytes, 256 * sizeof(double))) return rc;
    double *partial = (double *)ctx->scratch;
    hipLaunchKernelGGL(bf_iw_exp_kernel, dim3(nb), dim3(256), 0, ctx->stream, n, logp, logq, w, partial);
    hipLaunchKernelGGL(bf_iw_clip_kernel, dim3(nb), dim3(256), 0, ctx->stream, n, w, partial, nb, k_trunc, w_trunc);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
