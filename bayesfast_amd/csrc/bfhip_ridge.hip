// bfhip_ridge.hip -- the ridge path of the surrogate fit scored by exact leave-one-out (bfhip_ridge_path), and the rotation of the
// design into the eigenbasis that feeds it (bfhip_ridge_rotate).
//
// For a fixed penalty ridge regression is least squares on augmented data, so the residual of row i under a fit WITHOUT row i is
// still S_i / (1 - h_i).  With one symmetric eigen-decomposition (eigenvalues Lam_j, rows z_i of the rotated design, T = Z^T B')
//   h_i(lam) = h0_i + sum_j z_ij^2 g_j(lam),   fitted_i(lam) = sum_j z_ij T_j g_j(lam),   g_j = 1 / (Lam_j + lam)
// for every penalty of a path at once: a contraction (row tile x r) by (r x (m + 1) L) whose right operand T_jo g_jl is made from the
// (r, m) and (r, L) tables as it is used.  The complement form (more columns than rows: Z orthonormal, spanning what h0 leaves) sums
// 1 - h_i = sum_j z_ij^2 g_j and S_i = sum_j z_ij T_j g_j with g_j = lam / (Lam_j + lam) directly: no 1 - (...) that cancels.
#include "bfhip_block.h"
#include "bfhip_ridge.h"

// g (r, RG_LP): the weight of direction j at penalty l, zero beyond L
__global__ void bf_ridge_weights_kernel(int r, int L, int complement, const double *__restrict__ Lam,
                                        const double *__restrict__ lambdas, double *__restrict__ g) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)r * RG_LP) return;
    const int j = (int)(idx / RG_LP), l = (int)(idx % RG_LP);
    double v = 0.;
    if (l < L) {
        const double lam = lambdas[l];
        v = (complement ? lam : 1.) / (Lam[j] + lam);
    }
    g[idx] = v;
}

// the merge of two rows' (or row sets') sums: bfhip_loo.hip's, the first row of equal maxima
struct BfRidgeMerge {
    __device__ void operator()(double *a, const double *b) const {
        a[0] += b[0];
        a[1] += b[1];
        if (b[2] > a[2] || (b[2] == a[2] && b[3] < a[3])) {
            a[2] = b[2];
            a[3] = b[3];
        }
        a[4] += b[4];
        a[5] += b[5];
        a[6] += b[6];
    }
};

// Workgroup (tile, ob): rows 64 tile .. + 63 of Z (wave wv its rows 16 wv .. + 15), outputs 16 ob .. + 15, every penalty, RG_LC at a
// sweep.  Per step of four directions j the A operand of v_mfma_f64_16x16x4_f64 is z (lane (ci, kr): row ci, direction kr), the B
// operand T_jo g_jl for output ci (one accumulator tile per penalty of the sweep), and for the leverages z^2 against g_jl with the
// penalty on the column.  The accumulators hold rows kr + 4 reg, column ci; a row's 1 - h at penalty c of the sweep is in lane
// (c, kr) and is fetched by a shuffle.  Every sum has an order fixed by (n, r, m, L): j ascending inside the accumulators; a lane's
// four rows ascending, the four lane groups by a butterfly, the four waves in order; the tiles in order (bf_ridge_sums_kernel).
__global__ __launch_bounds__(256) void bf_ridge_path_kernel(int n, int r, int m, int L, int complement, const double *__restrict__ Z,
                                                          int ldz, const double *__restrict__ T, const double *__restrict__ g,
                                                          const double *__restrict__ Bp, const double *__restrict__ Bw,
                                                          const double *__restrict__ h0, const double *__restrict__ w, long row0,
                                                          double *__restrict__ h, double *__restrict__ part,
                                                          double *__restrict__ resid, double *__restrict__ e_loo) {
    __shared__ double red[RG_LC][4][RG_NS][RG_OB];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ci = lane & 15, kr = lane >> 4;
    const long ibase = (long)blockIdx.x * RG_ROWS + 16 * wv;
    const int o = (int)blockIdx.y * RG_OB + ci;
    const bool rok = ibase + ci < n, ook = o < m;
    const double *zrow = Z + (size_t)(rok ? ibase + ci : 0) * ldz;
    const double *tcol = T + (ook ? o : 0);
    for (int l0 = 0; l0 < L; l0 += RG_LC) {
        d4_t af[RG_LC], ah = (d4_t){0., 0., 0., 0.};
#pragma unroll
        for (int c = 0; c < RG_LC; ++c) af[c] = (d4_t){0., 0., 0., 0.};
#pragma unroll 2
        for (int k0 = 0; k0 < r; k0 += 4) {
            const bool jok = k0 + kr < r;
            const int j = jok ? k0 + kr : r - 1;   // (a step past the last direction reads it again and multiplies by zero)
            const double z = (rok && jok) ? zrow[j] : 0.;
            const double t = (ook && jok) ? tcol[(size_t)j * m] : 0.;
            const double *gj = g + (size_t)j * RG_LP + l0;
            ah = __builtin_amdgcn_mfma_f64_16x16x4f64(z * z, ci < RG_LC ? gj[ci] : 0., ah, 0, 0, 0);
#pragma unroll
            for (int c = 0; c < RG_LC; ++c) af[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(z, t * gj[c], af[c], 0, 0, 0);
        }
        // the epilogue: rows kr + 4 reg of the wave, output ci, the sweep's penalties
#pragma unroll
        for (int c = 0; c < RG_LC; ++c) {
            const int l = l0 + c;
            double v[RG_NS] = {0., 0., -1., 0., 0., 0., 0.};
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const double hv = __shfl(ah[reg], (lane & 48) | c, 64);
                const long i = ibase + kr + 4 * reg;
                if (l < L && i < n) {
                    double d, hh;
                    if (complement) {
                        d = hv;
                        hh = 1. - hv;
                    } else {
                        hh = (h0 ? h0[i] : 0.) + hv;
                        d = 1. - hh;
                    }
                    if (blockIdx.y == 0 && ci == c) h[(size_t)i * L + l] = hh;
                    if (ook) {
                        const size_t io = (size_t)i * m + o;
                        const double s = complement ? af[c][reg] : Bp[io] - af[c][reg];
                        const double wi = w ? w[i] : 1., y = Bw[io];
                        const bool ok = d > 0.;
                        const double inf = s < 0. ? -INFINITY : INFINITY;
                        const double sl = ok ? s / d : inf, el = ok ? s / (d * wi) : inf, al = fabs(el);
                        if (resid) {   // (L == 1)
                            resid[io] = s / wi;
                            e_loo[io] = el;
                        }
                        v[0] += s * s;
                        v[1] += sl * sl;
                        if (al > v[2]) {
                            v[2] = al;
                            v[3] = (double)(row0 + i);
                        }
                        v[4] += y;
                        v[5] += y * y;
                        v[6] += ok ? 0. : 1.;
                    }
                }
            }
            // the four lane groups of the wave (both operands of every merge are read before either is replaced)
#pragma unroll
            for (int mask = 16; mask <= 32; mask <<= 1) {
                double b[RG_NS];
#pragma unroll
                for (int k = 0; k < RG_NS; ++k) b[k] = bf_shfl_xor(v[k], mask);
                BfRidgeMerge()(v, b);
            }
            if (kr == 0)
#pragma unroll
                for (int k = 0; k < RG_NS; ++k) red[c][wv][k][ci] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < RG_LC * RG_OB) {
            const int c = threadIdx.x >> 4, oc = threadIdx.x & 15, l = l0 + c, oo = (int)blockIdx.y * RG_OB + oc;
            if (l < L && oo < m) {
                double a[RG_NS], b[RG_NS];
                for (int k = 0; k < RG_NS; ++k) a[k] = red[c][0][k][oc];
                for (int q = 1; q < 4; ++q) {
                    for (int k = 0; k < RG_NS; ++k) b[k] = red[c][q][k][oc];
                    BfRidgeMerge()(a, b);
                }
                double *p = part + (((size_t)blockIdx.x * L + l) * m + oo) * RG_NS;
                for (int k = 0; k < RG_NS; ++k) p[k] = a[k];
            }
        }
        __syncthreads();   // the slots are free for the next sweep
    }
}

// sums (L, m, BFHIP_LOO_NSUM): the tiles' partials folded in order, onto the sums of the rows before row0 when there are any
__global__ void bf_ridge_sums_kernel(int n_tiles, int L, int m, long row0, const double *__restrict__ part, double *__restrict__ sums) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long lm = (long)L * m;
    if (idx >= lm) return;
    double a[RG_NS] = {0., 0., -1., 0., 0., 0., 0.}, b[RG_NS];
    double *s = sums + (size_t)idx * BFHIP_LOO_NSUM;
    if (row0 > 0)
        for (int k = 0; k < RG_NS; ++k) a[k] = s[k];
    for (int t = 0; t < n_tiles; ++t) {
        const double *p = part + ((size_t)t * lm + idx) * RG_NS;
        for (int k = 0; k < RG_NS; ++k) b[k] = p[k];
        BfRidgeMerge()(a, b);
    }
    for (int k = 0; k < RG_NS; ++k) s[k] = a[k];
    s[RG_NS] = 0.;
}

extern "C" int bfhip_ridge_path(bfhip_ctx *ctx, int n, int r, int m, int L, const double *Z, int ldz, const double *Lam, const double *T,
                                const double *lambdas, const double *Bp, const double *Bw, const double *h0, const double *w,
                                int complement, long row0, double *h, double *sums, double *resid, double *e_loo, double *work,
                                size_t work_doubles) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || r < 1 || m < 1 || L < 1 || L > BFHIP_RIDGE_MAX_L || ldz < r || row0 < 0 || row0 % BFHIP_RIDGE_TILE != 0)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_ridge_path: invalid size (1 <= L <= %d, row0 a multiple of %d)", BFHIP_RIDGE_MAX_L,
                            BFHIP_RIDGE_TILE);
    if (!Z || !Lam || !T || !lambdas || !Bw || !h || !sums || !work || (!complement && !Bp))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_ridge_path: NULL array");
    if ((resid == NULL) != (e_loo == NULL) || (resid && L != 1))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_ridge_path: resid and e_loo are given together, and only for L = 1");
    if (work_doubles < (size_t)BFHIP_RIDGE_WORK(n, r, m, L))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_ridge_path: work holds %zu doubles, %zu needed", work_doubles,
                            (size_t)BFHIP_RIDGE_WORK(n, r, m, L));
    const int n_tiles = (n + RG_ROWS - 1) / RG_ROWS;
    double *g = work, *part = work + (size_t)r * RG_LP;
    const long ng = (long)r * RG_LP, lm = (long)L * m;
    hipLaunchKernelGGL(bf_ridge_weights_kernel, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, r, L, complement, Lam,
                       lambdas, g);
    hipLaunchKernelGGL(bf_ridge_path_kernel, dim3(n_tiles, (m + RG_OB - 1) / RG_OB), dim3(256), 0, ctx->stream, n, r, m, L, complement, Z,
                       ldz, T, g, Bp, Bw, h0, w, row0, h, part, resid, e_loo);
    hipLaunchKernelGGL(bf_ridge_sums_kernel, dim3((unsigned)((lm + 255) / 256)), dim3(256), 0, ctx->stream, n_tiles, L, m, row0, part,
                       sums);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// Z (n, r) = A (n, P) V (P, r): the rows of the design in the eigenbasis
// ---------------------------------------------------------------------------------------------------
// Workgroup (tile, cb): rows 64 tile .. + 63 (wave wv its rows 16 wv .. + 15), columns 64 cb .. + 63 as four accumulator tiles.  A
// row's sums run over k ascending whatever the launch's size: a row's Z does not depend on the rows it is rotated with.
__global__ __launch_bounds__(256) void bf_ridge_rotate_kernel(int n, int P, int r, const double *__restrict__ A, int lda,
                                                            const double *__restrict__ V, int ldv, double *__restrict__ Z, int ldz) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, ci = lane & 15, kr = lane >> 4;
    const long ibase = (long)blockIdx.x * RG_ROWS + 16 * wv;
    const int c0 = (int)blockIdx.y * 64;
    const bool rok = ibase + ci < n;
    const double *arow = A + (size_t)(rok ? ibase + ci : 0) * lda;
    d4_t acc[4];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) acc[bb] = (d4_t){0., 0., 0., 0.};
#pragma unroll 4
    for (int k0 = 0; k0 < P; k0 += 4) {
        const bool kok = k0 + kr < P;
        const int k = kok ? k0 + kr : P - 1;
        const double a = (rok && kok) ? arow[k] : 0.;
        const double *vk = V + (size_t)k * ldv;
#pragma unroll
        for (int bb = 0; bb < 4; ++bb) {
            const int c = c0 + 16 * bb + ci;
            acc[bb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (kok && c < r) ? vk[c] : 0., acc[bb], 0, 0, 0);
        }
    }
#pragma unroll
    for (int bb = 0; bb < 4; ++bb)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const long i = ibase + kr + 4 * reg;
            const int c = c0 + 16 * bb + ci;
            if (i < n && c < r) Z[(size_t)i * ldz + c] = acc[bb][reg];
        }
}

extern "C" int bfhip_ridge_rotate(bfhip_ctx *ctx, int n, int P, int r, const double *A, int lda, const double *V, int ldv, double *Z,
                                  int ldz) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || P < 1 || r < 1 || lda < P || ldv < r || ldz < r || !A || !V || !Z)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_ridge_rotate: invalid argument");
    hipLaunchKernelGGL(bf_ridge_rotate_kernel, dim3((n + RG_ROWS - 1) / RG_ROWS, (r + 63) / 64), dim3(256), 0, ctx->stream, n, P, r, A,
                       lda, V, ldv, Z, ldz);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
