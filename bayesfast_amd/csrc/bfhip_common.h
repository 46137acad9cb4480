// bfhip_common.h -- shared device/host definitions of libbfhip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/bfhip.h"
#include "bfhip_model.h"
#include "bfhip_tune.h"

// ---- wave helpers ---------------------------------------------------------------------------------
__device__ inline double bf_shfl_xor(double v, int mask) { return __shfl_xor(v, mask, 64); }

// numpy.logaddexp
__device__ inline double bf_logaddexp(double x, double y) {
    if (x == y) return x + 0.6931471805599453094;
    double tmp = x - y;
    if (tmp > 0) return x + log1p(exp(-tmp));
    if (tmp <= 0) return y + log1p(exp(tmp));
    return tmp;  // NaN
}

// float64 -> uint64 whose unsigned order is the numeric order, every NaN last and -0 == +0 (numpy's sort order)
__device__ inline uint64_t bf_order_key(double v) {
    if (v != v) return ~0ull;
    if (v == 0.) v = 0.;
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
// the value behind such a key: -0 comes back as +0, every NaN as one NaN
__device__ inline double bf_order_value(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

#define BF_HIP_CHECK(expr)                                                                 \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) return bf_set_error(BFHIP_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

int bf_set_error(int code, const char *fmt, ...);

struct bfhip_ctx {
    int device;
    hipStream_t stream;
    int has_model;
    DevModel model;
    void *model_buf;      // one device allocation holding pd + fragments
    size_t model_bytes;
    void *cubic_buf;      // cubic-term tables
    size_t cubic_bytes;
    void *pm_buf;         // multi-output polymodel (bfhip_polymodel_upload)
    size_t pm_bytes;
    int has_pm;
    void *pld_buf;        // pipeline density (bfhip_pipeline_upload): fragments, tables
    size_t pld_bytes;
    struct PolyDev {
        int d, DP, m, use_bound, has_quad;
        const double *Sf;    // [m][DP*DP] A fragments of S_o = A_o + A_o^T
        const double *lin;   // [m][DP]
        const double *c0;    // [m]
        const double *f_mu;  // [m]
        const double *mu;    // [DP]
        const double *Hf;    // [DP*DP]
        double alpha;
        // cubic configs, compact over their masks (per output o: A2[o][n2][n2], A2t[o], T3t[o][n3][n3][n3] as in DevModel)
        int n2, n3;
        const int *mask2, *pos2, *mask3, *pos3;
        const double *A2, *A2t, *T3t;
    } pm;
    int *tail_buf;        // the chains of a launch's tail: count, then their indices (bfhip_sampler.hip: launch_nuts_pipe)
    size_t tail_bytes;
    void *scratch;        // sampler tree scratch (grow-only)
    size_t scratch_bytes;
    int n_cu;
    void *flow;           // counters and exchange buffers of the triangular solves (bfhip_fit.hip: ensure_flow)
    size_t flow_bytes;
    void *hess_work;      // per-workgroup slots of the pipeline density's Hessian (bfhip_pld_hess.h: G and G^T G; grow-only)
    size_t hess_work_bytes;
};

// Every entry point that launches or allocates runs on its context's device, whatever the caller's current device is
// (one process may hold contexts of several GPUs); the previous device is restored on return.
struct BfDeviceGuard {
    int prev = -1;
    explicit BfDeviceGuard(const bfhip_ctx *ctx) {
        if (ctx && hipGetDevice(&prev) == hipSuccess && prev != ctx->device) (void)hipSetDevice(ctx->device);
        else prev = -1;
    }
    ~BfDeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// ---- host-side launch plumbing ----------------------------------------------------------------------
#define BF_LDS_MAX ((size_t)160 * 1024)   // dynamic LDS of one workgroup on gfx950

// Opts a kernel into more than 64 KB of dynamic LDS.  The attribute belongs to the kernel on the current device, so it is raised
// at every call rather than remembered (one process may drive several GPUs).
template <typename K>
static inline int bf_set_lds(K kern, size_t bytes) {
    if (bytes > 64 * 1024)
        BF_HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

// Grow-only device buffer: at least need bytes at *buf, *bytes its size.  Growing waits for the context's stream (nothing
// may still use the old buffer); allocation is outside any timed region after the first call.
static inline int bf_grow(bfhip_ctx *ctx, void **buf, size_t *bytes, size_t need) {
    if (*bytes >= need) return 0;
    BF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (*buf) BF_HIP_CHECK(hipFree(*buf));
    *buf = NULL;
    *bytes = 0;
    BF_HIP_CHECK(hipMalloc(buf, need));
    *bytes = need;
    return 0;
}

// ---- shared by the statistics files ------------------------------------------------------------------------
// bfhip_refit.hip: stable radix sort (rocPRIM) of the order keys of a[i * stride + col], i < n, with the permutation as Index
// (int64_t: bfhip_sort_keys, uint32_t: bfhip_diag_sort).  Unsorted keys, indices and rocPRIM's temporary storage live in
// ctx->scratch, each padded to 256 bytes.  The caller has checked its arguments, 1 <= n <= 2^31 - 1.
template <typename Index>
int bf_sort_column(bfhip_ctx *ctx, long n, const double *a, long stride, int col, uint64_t *keys_sorted, Index *order);
// bfhip_diag.hip: the gather of a batch of columns of the (chain, time, dimension) tensor into n_el = rows x 16 doubles, a chain
// cut into `split` pieces of h steps (2: bfhip_diag_columns, 1: bfhip_wstat_columns).  x is offset by off elements; the caller
// has checked its arguments.
int bf_columns_launch(bfhip_ctx *ctx, int split, long n_el, long h, long ldw, long ldr, const void *x, int is_f32, long off, int nb,
                      int mode, const double *c, const double *w, double *out);

// the common surrogate: linear + quadratic configs with the extrapolation bound; decay term and constraint transform optional
static inline bool bf_common_surrogate(const DevModel &m) {
    return m.has_quad && m.use_bound && !m.has_su && !m.has_cubic && !m.has_link;
}
// ... with neither of the optional terms
static inline bool bf_model_plain(const DevModel &m) { return bf_common_surrogate(m) && !m.use_decay && !m.has_transform; }
// the feature-set bits of the compile-time instantiations: 1 | decay << 1 | transform << 2 (the pipeline density: 8 | transform << 2)
static inline int bf_feature_bits(const DevModel &m) {
    return m.pld.on ? (8 | (m.has_transform ? 4 : 0)) : (1 | (m.use_decay ? 2 : 0) | (m.has_transform ? 4 : 0));
}
