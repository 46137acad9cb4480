// bfhip_loo.hip -- leave-one-out validation of the least-squares fit (bfhip_lstsq_loo): the leverages of the design rows from the
// kept Cholesky factor, and the leave-one-out residuals with their per-output sums.
//
// For linear least squares the residual of point i under a fit WITHOUT point i is e_i / (1 - h_i) exactly, with the leverage
// h_i = a_i^T (A^T A)^-1 a_i = | L^-1 D a_i |^2 for the factor D L L^T D of the Gram matrix the fit keeps.  The leverages are
// n P^2 FP64 operations (a few times the fit itself): a forward substitution with n right-hand sides, on the matrix cores.
#include "bfhip_block.h"
#include "bfhip_loo.h"

#define LV_NB 64               // block of the factor (NB_ of bfhip_fit.hip)
#define LV_W BFHIP_LOO_TILE    // design rows per workgroup: the columns of its right-hand side
#define LV_LD 80               // LDS row stride in doubles: rows kr and kr + 1 of a k-step start 32 banks apart
static_assert(LV_W == 64, "one wave's lanes load one row of a Z block");

// One workgroup owns LV_W design rows i0 .. i0 + 63 as the columns of a right-hand side and walks the 64-row blocks of L in order:
//   Z_b = Linv_bb ((D a)_b - sum_{k < b} L_bk Z_k),     h_i = sum_b | column i of Z_b |^2.
// Its finished Z_k (64 x 64, row-major) sit in its own slice of the workspace, Z = ws + blockIdx.x * nb * 4096; nothing is exchanged
// between workgroups.  Wave wv owns rows 16 wv .. 16 wv + 15 of the block: the A operand of v_mfma_f64_16x16x4 is its 16 rows of
// L_bk, read straight from the transposed block (k, b) in the upper triangle of G (lane (ci, kr) takes G[(k0 + 4 s + kr) P + b0 +
// 16 wv + ci]: 16 consecutive doubles per kr), the B operand Z_k from LDS, shared by the four waves.  The loads of step k + 1 are
// in flight under the products of step k (a register of L_bk is asked for again as soon as its product is issued).  Rows of the last block beyond P: the factor's padding there is the identity (bf_chol_*
// kernels), so with a zero right-hand side and zero L_bk rows they stay zero and add nothing.
// Every sum has a fixed order (k ascending inside the MFMA accumulators; blocks b ascending, then the four accumulator rows; then
// the 16 (wave, kr) partials in order): a row's leverage depends neither on the launch's size nor on the tile it falls in.
__global__ __launch_bounds__(256, 2) void bf_leverage_kernel(int n, int P, int tile0, const double *__restrict__ A, int lda,
                                                        const double *__restrict__ G, const double *__restrict__ dsc,
                                                        const double *__restrict__ LinvAll, const int *__restrict__ info, double *ws,
                                                        double *__restrict__ h) {
    __shared__ __attribute__((aligned(16))) double Zs[LV_NB][LV_LD];
    __shared__ double hp[16][LV_W];
    if (*info != 0) return;  // (uniform: a failed factorisation leaves h untouched)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ci = lane & 15, kr = lane >> 4;
    const int nb = (P + LV_NB - 1) / LV_NB;
    const long i0 = (long)(tile0 + (int)blockIdx.x) * LV_W;
    double *Z = ws + (size_t)blockIdx.x * nb * (LV_NB * LV_W);
    double hs[4] = {0., 0., 0., 0.};
    for (int b = 0; b < nb; ++b) {
        const int b0 = b * LV_NB;
        d4_t acc[4];
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) acc[bb] = (d4_t){0., 0., 0., 0.};
        double pa[16], pz[16];
        const bool cok = b0 + 16 * wv + ci < P;
        const double *Gb = G + (size_t)kr * P + b0 + 16 * wv + ci;   // lane (ci, kr)'s element of row 4 s + kr of block (k, b): + (64 k + 4 s) P
        auto fetch_z = [&](int k) {
            const double *Zk = Z + (size_t)k * (LV_NB * LV_W);
#pragma unroll
            for (int e = 0; e < 16; ++e) pz[e] = Zk[(wv + 4 * e) * LV_W + lane];
        };
        if (b > 0) {
#pragma unroll
            for (int s = 0; s < 16; ++s) pa[s] = cok ? Gb[(size_t)(4 * s) * P] : 0.;
            fetch_z(0);
        }
        for (int k = 0; k < b; ++k) {
            __syncthreads();  // every wave is through with the block before this one
#pragma unroll
            for (int e = 0; e < 16; ++e) Zs[wv + 4 * e][lane] = pz[e];
            // the next step's operands are asked for as this step's are used up (the last step asks for its own again: no branch)
            const int kn = k + 1 < b ? k + 1 : k;
            fetch_z(kn);
            const double *Gn = Gb + (size_t)(kn * LV_NB) * P;
            __syncthreads();
#pragma unroll
            for (int s = 0; s < 16; ++s) {
#pragma unroll
                for (int bb = 0; bb < 4; ++bb)
                    acc[bb] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[s], Zs[4 * s + kr][16 * bb + ci], acc[bb], 0, 0, 0);
                pa[s] = cok ? Gn[(size_t)(4 * s) * P] : 0.;
            }
        }
        // (D a)_b, element (row b0 + lane, column wv + 4 e): coalesced along the design row (once per block: its latency is one k-step's)
        double da[16];
        {
            const bool rok = b0 + lane < P;
            const double dl = rok ? dsc[b0 + lane] : 0.;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const long i = i0 + wv + 4 * e;
                da[e] = (rok && i < n) ? dl * A[(size_t)i * lda + b0 + lane] : 0.;
            }
        }
        __syncthreads();
        // T = (D a)_b - sum_k L_bk Z_k in LDS (the accumulators hold rows 16 wv + kr + 4 r, columns 16 bb + ci)
#pragma unroll
        for (int e = 0; e < 16; ++e) Zs[lane][wv + 4 * e] = da[e];
        __syncthreads();
#pragma unroll
        for (int bb = 0; bb < 4; ++bb)
#pragma unroll
            for (int r = 0; r < 4; ++r) Zs[16 * wv + kr + 4 * r][16 * bb + ci] -= acc[bb][r];
        __syncthreads();
        // Z_b = Linv_bb T (Linv is lower triangular: rows 16 wv .. 16 wv + 15 end at column 16 wv + 15)
        const double *Li = LinvAll + (size_t)b * (LV_NB * LV_NB) + (16 * wv + ci) * LV_NB + kr;
        d4_t z[4];
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) z[bb] = (d4_t){0., 0., 0., 0.};
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (s <= 4 * wv + 3) {
                const double fl = Li[4 * s];
#pragma unroll
                for (int bb = 0; bb < 4; ++bb)
                    z[bb] = __builtin_amdgcn_mfma_f64_16x16x4f64(fl, Zs[4 * s + kr][16 * bb + ci], z[bb], 0, 0, 0);
            }
        double *Zb = Z + (size_t)b * (LV_NB * LV_W);
#pragma unroll
        for (int bb = 0; bb < 4; ++bb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (b + 1 < nb) Zb[(16 * wv + kr + 4 * r) * LV_W + 16 * bb + ci] = z[bb][r];  // (the last block is read by nobody)
                hs[bb] += z[bb][r] * z[bb][r];
            }
        __syncthreads();  // Z_b is in the slice before any wave's fetch of the next block reads it (the slice is this workgroup's alone)
    }
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) hp[4 * wv + kr][16 * bb + ci] = hs[bb];
    __syncthreads();
    if (threadIdx.x < LV_W && i0 + threadIdx.x < n) {
        double s = 0.;
        for (int p = 0; p < 16; ++p) s += hp[p][threadIdx.x];
        h[i0 + threadIdx.x] = s;
    }
}

int bf_leverage_launch(bfhip_ctx *ctx, int n, int P, const double *A, int lda, const double *G, const double *dsc,
                       const double *LinvAll, const int *info, double *h, double *ws, size_t ws_doubles) {
    const int nb = (P + LV_NB - 1) / LV_NB;
    const size_t slice = (size_t)nb * (LV_NB * LV_W);
    if (ws_doubles > (size_t)BFHIP_LOO_WS_MAX) ws_doubles = (size_t)BFHIP_LOO_WS_MAX;
    const int n_tiles = (n + LV_W - 1) / LV_W;
    size_t fl = ws_doubles / slice;
    if (fl < 1) return bf_set_error(BFHIP_ERR_ARG, "bfhip_lstsq_loo: the workspace holds no tile (%zu doubles needed)", slice);
    const int in_flight = fl < (size_t)n_tiles ? (int)fl : n_tiles;
    // passes of equal size: the tiles of a pass run side by side, a pass starts when the one before it has left the workspace
    const int n_pass = (n_tiles + in_flight - 1) / in_flight;
    const int per_pass = (n_tiles + n_pass - 1) / n_pass;
    for (int t0 = 0; t0 < n_tiles; t0 += per_pass) {
        const int nt = n_tiles - t0 < per_pass ? n_tiles - t0 : per_pass;
        hipLaunchKernelGGL(bf_leverage_kernel, dim3(nt), dim3(256), 0, ctx->stream, n, P, t0, A, lda, G, dsc, LinvAll, info, ws, h);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Leave-one-out residuals and the per-output sums
// ---------------------------------------------------------------------------------------------------
// e_loo[i][q] = S[i][q] / ((1 - h_i) w_i): the held-out residual in the units of y.  A row whose 1 - h_i is not positive after
// rounding (the fit passes through it whatever its value) gets an infinite one, with the sign of S
__device__ inline double bf_loo_value(double s, double hi, double wi) {
    const double d = 1. - hi;
    if (!(d > 0.)) return s < 0. ? -INFINITY : INFINITY;
    return s / (d * wi);
}
__global__ void bf_loo_resid_kernel(int n, int m, const double *__restrict__ S, const double *__restrict__ h,
                                    const double *__restrict__ w, const int *__restrict__ info, double *__restrict__ e_loo) {
    if (*info != 0) return;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * m) return;
    const long i = idx / m;
    e_loo[idx] = bf_loo_value(S[idx], h[i], w ? w[i] : 1.);
}

// the sums of output q = blockIdx.x (BFHIP_LOO_*): thread t takes rows t, t + 256, ... in order, then the block tree
struct BfLooMerge {
    __device__ void operator()(double *a, const double *b) const {
        a[0] += b[0];
        a[1] += b[1];
        if (b[2] > a[2] || (b[2] == a[2] && b[3] < a[3])) {  // (the first row of equal maxima)
            a[2] = b[2];
            a[3] = b[3];
        }
        a[4] += b[4];
        a[5] += b[5];
        a[6] += b[6];
    }
};
__global__ __launch_bounds__(256) void bf_loo_sums_kernel(int n, int m, const double *__restrict__ S, const double *__restrict__ B,
                                                        const double *__restrict__ h, const double *__restrict__ e_loo,
                                                        const int *__restrict__ info, double *__restrict__ sums) {
    __shared__ double slot[7 * 256];
    if (*info != 0) return;
    const int q = blockIdx.x, t = threadIdx.x;
    double v[7] = {0., 0., -1., 0., 0., 0., 0.};
    for (int i = t; i < n; i += 256) {
        const double s = S[(size_t)i * m + q], y = B[(size_t)i * m + q], d = 1. - h[i];
        const double sl = d > 0. ? s / d : (s < 0. ? -INFINITY : INFINITY);
        const double al = fabs(e_loo[(size_t)i * m + q]);
        v[0] += s * s;
        v[1] += sl * sl;
        if (al > v[2]) {
            v[2] = al;
            v[3] = (double)i;
        }
        v[4] += y;
        v[5] += y * y;
        v[6] += d > 0. ? 0. : 1.;
    }
    bf_block_tree<256, 7>(v, slot, BfLooMerge());
    if (t < BFHIP_LOO_NSUM) sums[(size_t)q * BFHIP_LOO_NSUM + t] = t < 7 ? v[t] : 0.;
}

int bf_loo_sums_launch(bfhip_ctx *ctx, int n, int m, const double *S, const double *B, const double *h, const double *w,
                       const int *info, double *e_loo, double *sums) {
    const long ne = (long)n * m;
    hipLaunchKernelGGL(bf_loo_resid_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, ctx->stream, n, m, S, h, w, info, e_loo);
    hipLaunchKernelGGL(bf_loo_sums_kernel, dim3(m), dim3(256), 0, ctx->stream, n, m, S, B, h, e_loo, info, sums);
    return 0;
}
