// bfhip_rw.h -- the posterior reweighted to a batch of 16 columns of log ratios (bayesfast_amd/utils/reweight.py has the definitions);
// included at the end of bfhip_psis.hip, after bfhip_ploo.h, whose first two stages it follows: with -l in the series buffer in mode
// BFHIP_PLOO_ELL their ratio lb - ell is r = lb + l, so bfhip_ploo_moments gives max r and the flags and bfhip_ploo_tail the M + 1
// largest pairs of every column.
//
//   bfhip_rw_finish   the fit per column and the smoothed tail as bfhip_ploo_finish launches them (pl_fit_and_smooth), then per column
//                     and parameter j < d the sums  sum e, sum e (x_j - c_j), sum e (x_j - c_j)^2  and the same three with e^2,
//                     e = exp(smoothed shifted r), over the draws read in place.  Where fewer than M + 1 rows have any weight the
//                     tail holds rows of zero weight, to which the fit hands smoothed weight: they are in no sum of the table (a
//                     1 + 2 d-th feature collects them), and in sum e and sum e^2 behind ess and the evidence ratio, as in bfhip_psis.
//
// The body pass is a (16 x n) by (n x (1 + 2 d)) product on the FP64 matrix cores: a wave takes four rows at a time, lane l holds
// A[column l & 15][row l >> 4] = e (0 for a row above the cut pair -- it comes with its smoothed value -- and for a row of zero weight)
// and B[row l >> 4][feature l & 15] of the features [1, x - c, (x - c)^2] in tiles of 16 (all 0 in a row of zero weight, which is not
// read as a number), and one v_mfma_f64_16x16x4_f64 per tile and stream adds the sixteen columns' sums: D[column (l >> 4) + 4 reg]
// [feature l & 15].  A workgroup's four waves are folded in order, the workgroups by the finish kernel in 16 slices folded in order, the
// M tail rows -- fetched by index -- in RW_TAILS slices folded in order: every order is set by n and d alone, nothing is atomic, and an entry of D
// sees its own row of A alone, so a column's sums are the same bits in any slot of any batch.
#pragma once

#define RW_MAXG 768     // workgroups of the body pass along the rows (three fit a compute unit of the 256: its LDS and registers); a
                        // workgroup takes 16 rows (4 waves x 4) per step
#define RW_TG 4         // tiles of 16 features per workgroup: blockIdx.y walks the groups (eight accumulators of four doubles)
#define RW_TAILS 32     // slices of the tail rows, at most, each of four sub-slices
#define RW_HEAD BFHIP_RW_SUMS   // rows of the out block before the sums
static_assert(PS_T == 256 && PL_B == 16, "four waves; a tile is 16 columns x 16 features");

typedef double rw_d4 __attribute__((ext_vector_type(4)));

struct RwDraws {   // series row s is draw (s / n_draw, s % n_draw) at x[(s / n_draw) ldw + (s % n_draw) ldr + j] (since is in x already)
    long n_draw, ldw, ldr;
    const void *x;
    int d;
    const double *c;
};

// feature f of [1, x - c, (x - c)^2]: kind 0 the one, 1 and 2 parameter col, 3 padding
__device__ inline void rw_feature(int f, int d, int &kind, int &col) {
    kind = f == 0 ? 0 : f <= d ? 1 : f <= 2 * d ? 2 : 3;
    col = kind == 1 ? f - 1 : kind == 2 ? f - d - 1 : 0;
}
template <typename T>
__device__ inline double rw_value_at(const RwDraws &q, long off, int kind, int col, double cj) {   // off: the draw's first element
    if (kind == 0) return 1.;
    if (kind == 3) return 0.;
    const double dx = (double)((const T *)q.x)[off + col] - cj;
    return kind == 1 ? dx : dx * dx;
}
template <typename T>
__device__ inline double rw_value(const RwDraws &q, long row, int kind, int col, double cj) {
    const long ch = row / q.n_draw, i = row - ch * q.n_draw;
    return rw_value_at<T>(q, ch * q.ldw + i * q.ldr, kind, col, cj);
}

static inline int rw_grid(long n) {
    const long g = (n + 15) / 16;
    return (int)(g < 1 ? 1 : (g > RW_MAXG ? RW_MAXG : g));
}
static inline int rw_tails(long M) {
    const long s = (M + 63) / 64;
    return (int)(s < 1 ? 1 : (s > RW_TAILS ? RW_TAILS : s));
}

struct RwWork {
    double *part;    // G x 2 streams x F features (tiles of 16, padded) x 16 columns
    double *tpart;   // 16 columns x slices x 2 streams x F
    int G, ns, ntile, F;
    size_t bytes;
};
static RwWork rw_work(void *work, long n, int d) {
    RwWork w;
    w.G = rw_grid(n);
    w.ns = rw_tails(pl_tail_size(n));
    w.ntile = (1 + 2 * d + 15) / 16;
    w.F = 16 * w.ntile;
    const size_t body = ((size_t)w.G * 2 * w.F * PL_B * sizeof(double) + 255) / 256 * 256;
    const size_t tail = ((size_t)PL_B * w.ns * 2 * w.F * sizeof(double) + 255) / 256 * 256;
    w.part = (double *)work;
    w.tpart = (double *)((char *)work + body);
    w.bytes = body + tail;
    return w;
}

extern "C" size_t bfhip_rw_work_bytes(long n, int d) {
    return n < 1 || n > 0x7fffffffL || d < 1 || d > BFHIP_MAX_DIM ? 0 : rw_work(nullptr, n, d).bytes;
}

// ---- the rows not above the cut pair -------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(PS_T) void rw_body_kernel(PlCols a, long M, const double *__restrict__ out, const uint64_t *__restrict__ tail_keys,
                                                      const uint32_t *__restrict__ tail_idx, RwDraws q, int ntile, double *__restrict__ part) {
    __shared__ double red[3][2 * RW_TG * 4][64];   // waves 1 .. 3: their accumulators, lane by lane
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (the wave's steps are scalar work)
    const int b = lane & 15, k = lane >> 4;        // A: column b, row k of the step.  B: row k, feature b of the tile
    const int t0 = blockIdx.y * RW_TG, nt = ntile - t0 < RW_TG ? ntile - t0 : RW_TG;
    const bool col_on = b < a.nb;
    const double lb0 = -log((double)a.n);
    const double mx = col_on ? out[PL_MAXR * PL_B + b] : 0.;
    const uint64_t kc = col_on ? tail_keys[(long)b * (M + 1)] : 0;   // the cut pair
    const uint32_t ic = col_on ? tail_idx[(long)b * (M + 1)] : 0;
    int kind[RW_TG], col[RW_TG];
    double cj[RW_TG];
#pragma unroll
    for (int t = 0; t < RW_TG; ++t) {
        rw_feature(t < nt ? 16 * (t0 + t) + b : 2 * q.d + 1, q.d, kind[t], col[t]);
        cj[t] = kind[t] == 1 || kind[t] == 2 ? q.c[col[t]] : 0.;
    }
    rw_d4 acc[2][RW_TG];
#pragma unroll
    for (int t = 0; t < RW_TG; ++t) acc[0][t] = acc[1][t] = rw_d4{0., 0., 0., 0.};
    const long nstep = (a.n + 3) / 4;
    for (long s = (long)blockIdx.x * 4 + wave; s < nstep; s += (long)gridDim.x * 4) {   // (the same trip count in every lane of a wave)
        const long row = 4 * s + k;
        long ch = (4 * s) / q.n_draw, i = 4 * s - ch * q.n_draw + k;   // one division per wave and step; the lane's row follows
        while (i >= q.n_draw) {
            i -= q.n_draw;
            ++ch;
        }
        const long off = ch * q.ldw + i * q.ldr;
        double lb = -__builtin_inf();
        if (row < a.n) lb = a.lb ? a.lb[row] : lb0;
        const bool live = lb != -__builtin_inf();   // a row of the sample
        double e = 0.;
        if (live && col_on) {
            const double rs = pl_shifted(a.lb ? lb : 0., pl_ell(a, row, b), mx);
            const uint64_t key = bf_order_key(rs);
            if (!(key > kc || (key == kc && (uint32_t)row > ic))) e = exp(rs);
        }
        const double e2 = e * e;
#pragma unroll
        for (int t = 0; t < RW_TG; ++t) {
            if (t >= nt) continue;
            const double v = live ? rw_value_at<T>(q, off, kind[t], col[t], cj[t]) : 0.;
            acc[0][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(e, v, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(e2, v, acc[1][t], 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int st = 0; st < 2; ++st)
#pragma unroll
            for (int t = 0; t < RW_TG; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave - 1][(st * RW_TG + t) * 4 + r][lane] = acc[st][t][r];
    }
    __syncthreads();
    if (wave != 0) return;
    const int F = 16 * ntile;
#pragma unroll
    for (int st = 0; st < 2; ++st)
#pragma unroll
        for (int t = 0; t < RW_TG; ++t) {
            if (t >= nt) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double v = acc[st][t][r];
                for (int w = 0; w < 3; ++w) v += red[w][(st * RW_TG + t) * 4 + r][lane];
                // D: column k + 4 r, feature b of tile t0 + t
                part[(((size_t)blockIdx.x * 2 + st) * F + 16 * (t0 + t) + b) * PL_B + k + 4 * r] = v;
            }
        }
}

// ---- the M tail rows, fetched by index, with their smoothed values: workgroup (column b, slice), thread (feature, sub-slice) ----------
template <typename T>
__global__ __launch_bounds__(PS_T) void rw_tail_kernel(PlCols a, long M, int F, int nf, const uint32_t *__restrict__ tail_idx,
                                                      const double *__restrict__ sm, RwDraws q, double *__restrict__ tpart) {
    __shared__ double red[2][PS_T];
    const int b = blockIdx.x, slice = blockIdx.y, ns = gridDim.y, fl = threadIdx.x & 63, sub = threadIdx.x >> 6;
    const double lb0 = -log((double)a.n);
    for (int f0 = 0; f0 <= nf; f0 += 64) {   // feature nf: the one of the rows of zero weight (fewer than M + 1 rows have any)
        const int f = f0 + fl;
        int kind, col;
        rw_feature(f < nf ? f : 2 * q.d + 1, q.d, kind, col);
        const double cj = kind == 1 || kind == 2 ? q.c[col] : 0.;
        double s1 = 0., s2 = 0.;
        if (f <= nf)
            for (long i = (long)slice * 4 + sub; i < M; i += (long)ns * 4) {
                const double e = exp(sm[(long)b * (M + 1) + i]);
                const long row = tail_idx[(long)b * (M + 1) + 1 + i];
                bool dead = row >= a.n;   // (the caller's array: nothing is read through an index that is no row)
                if (!dead) dead = (a.lb ? a.lb[row] : lb0) == -__builtin_inf();
                if (dead != (f == nf)) continue;
                const double v = dead ? 1. : rw_value<T>(q, row, kind, col, cj);
                s1 += e * v;
                s2 += (e * e) * v;
            }
        red[0][threadIdx.x] = s1;
        red[1][threadIdx.x] = s2;
        __syncthreads();
        if (sub == 0 && f <= nf) {
            for (int w = 1; w < 4; ++w) {
                s1 += red[0][64 * w + fl];
                s2 += red[1][64 * w + fl];
            }
            tpart[(((size_t)b * ns + slice) * 2 + 0) * F + f] = s1;
            tpart[(((size_t)b * ns + slice) * 2 + 1) * F + f] = s2;
        }
        __syncthreads();
    }
}

// ---- workgroup (column b, 16 of the 2 (1 + 2 d) sums): thread (sum, slice) adds the body's workgroups slice, slice + 16, ..., slice 0
// folds the slices in order and adds the tail's slices in order; the first workgroup of a column holds sum e and sum e^2 (positions 0
// and 1: position p >= 2 is stream (p - 2) / 2 d, feature 1 + (p - 2) % 2 d) and writes the column's figures
__global__ __launch_bounds__(PS_T) void rw_finish_kernel(long M, int G, int F, int ns, int nf, const double *__restrict__ part,
                                                        const double *__restrict__ tpart, const double *__restrict__ out8s,
                                                        const double *__restrict__ out, double *__restrict__ rw) {
    __shared__ double red[PS_T];
    __shared__ double s12[2];
    const int b = blockIdx.x, j = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    const int p = 16 * blockIdx.y + j;
    const bool on = p < 2 * nf;
    const int st = p < 2 ? p : (p - 2) / (nf - 1), f = p < 2 ? 0 : 1 + (p - 2) % (nf - 1);
    const double nan = __builtin_nan("");
    const int own = (int)out[PL_FLAGS * PL_B + b];
    const bool bad = (own & 5) != 0;
    double v = 0.;
    if (on)
        for (int g = sl; g < G; g += BF_SLICES) v += part[(((size_t)g * 2 + st) * F + f) * PL_B + b];
    red[threadIdx.x] = v;
    __syncthreads();
    if (sl == 0 && on) {
        const double body = bf_slice_fold(v, 1, red, j, BfSum());
        double tail = 0.;
        for (int s = 0; s < ns; ++s) tail += tpart[(((size_t)b * ns + s) * 2 + st) * F + f];
        const double tot = body + tail;
        rw[(long)(RW_HEAD + st * nf + f) * PL_B + b] = bad ? nan : tot;
        if (p < 2) s12[p] = tot;
    }
    __syncthreads();
    if (threadIdx.x != 0 || blockIdx.y != 0) return;
    const double *out8 = out8s + 8 * b;
    const int flags = bad ? own : own | ((int)out8[7] & 2);
    double s1 = 0., s2 = 0.;   // with the rows of zero weight that the tail holds: psis's normalisation
    for (int s = 0; s < ns; ++s) {
        s1 += tpart[(((size_t)b * ns + s) * 2 + 0) * F + nf];
        s2 += tpart[(((size_t)b * ns + s) * 2 + 1) * F + nf];
    }
    s1 = s12[0] + s1;
    s2 = s12[1] + s2;
    rw[BFHIP_RW_LER * PL_B + b] = bad ? nan : out[PL_MAXR * PL_B + b] + log(s1);
    rw[BFHIP_RW_KHAT * PL_B + b] = bad ? nan : out8[0];
    rw[BFHIP_RW_SIGMA * PL_B + b] = bad ? nan : out8[1];
    rw[BFHIP_RW_M * PL_B + b] = (double)M;
    rw[BFHIP_RW_ESS * PL_B + b] = bad ? nan : s1 * s1 / s2;
    rw[BFHIP_RW_FLAGS * PL_B + b] = (double)flags;
    rw[BFHIP_RW_CUT * PL_B + b] = bad ? nan : out8[3];
    rw[(RW_HEAD - 1) * PL_B + b] = 0.;
}

template <typename T>
static void rw_launch(hipStream_t st, const PlCols &a, long M, const RwWork &rw, const PlWork &w, const RwDraws &q, const double *out,
                      const uint64_t *tail_keys, const uint32_t *tail_idx, double *rw_out) {
    const int nf = 1 + 2 * q.d;
    hipLaunchKernelGGL(rw_body_kernel<T>, dim3(rw.G, (rw.ntile + RW_TG - 1) / RW_TG), dim3(PS_T), 0, st, a, M, out, tail_keys, tail_idx, q,
                       rw.ntile, rw.part);
    hipLaunchKernelGGL(rw_tail_kernel<T>, dim3(a.nb, rw.ns), dim3(PS_T), 0, st, a, M, rw.F, nf, tail_idx, (const double *)w.sm, q, rw.tpart);
    hipLaunchKernelGGL(rw_finish_kernel, dim3(a.nb, (2 * nf + 15) / 16), dim3(PS_T), 0, st, M, rw.G, rw.F, rw.ns, nf, (const double *)rw.part,
                       (const double *)rw.tpart, (const double *)w.out8, out, rw_out);
}

extern "C" int bfhip_rw_finish(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                               const uint64_t *tail_keys, const uint32_t *tail_idx, const double *out, void *work, size_t work_bytes,
                               int n_chain, long n_draw, long ldw, long ldr, const void *x, int is_f32, long since, int d,
                               const double *centre, double *rw_out, void *rw_work_buf, size_t rw_work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (int rc = pl_check("bfhip_rw_finish", ctx, n, series, ld, nb, mode, c)) return rc;
    if (!out || !tail_keys || !tail_idx || !work || work_bytes < bfhip_ploo_work_bytes(n) || n_chain < 1 || n_draw < 1 ||
        (long)n_chain * n_draw != n || !x || since < 0 || d < 1 || d > BFHIP_MAX_DIM || ldr < d || (n_chain > 1 && ldw < 1) || !centre ||
        !rw_out || !rw_work_buf || rw_work_bytes < bfhip_rw_work_bytes(n, d))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_rw_finish: invalid argument");
    const long M = pl_tail_size(n);
    const int m = 30 + (int)floor(sqrt((double)M));
    if (m > PS_MAXM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_rw_finish: %d candidate thetas", m);
    const PlWork w = pl_work(work, n);
    const RwWork rw = rw_work(rw_work_buf, n, d);
    const PlCols a = {n, series, ld, nb, mode, c, lb};
    hipStream_t st = ctx->stream;
    pl_fit_and_smooth(st, w, nb, M, m, tail_keys);
    const size_t off = (size_t)since * (size_t)ldr;
    if (is_f32) {
        const RwDraws q = {n_draw, ldw, ldr, (const float *)x + off, d, centre};
        rw_launch<float>(st, a, M, rw, w, q, out, tail_keys, tail_idx, rw_out);
    } else {
        const RwDraws q = {n_draw, ldw, ldr, (const double *)x + off, d, centre};
        rw_launch<double>(st, a, M, rw, w, q, out, tail_keys, tail_idx, rw_out);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
