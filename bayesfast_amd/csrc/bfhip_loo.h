// bfhip_loo.h -- the launches of bfhip_loo.hip, called by bfhip_lstsq_loo (bfhip_fit.hip) once the factor is there.
#pragma once
#include "bfhip_common.h"

// h (n,) = | L^-1 D a_i |^2 from the kept factor (layout: include/bfhip.h, bfhip_solve_spd); ws holds ws_doubles doubles, at least
// one tile's slice (ceil(P / 64) * 64 * BFHIP_LOO_TILE).  Nothing is written when *info != 0.
int bf_leverage_launch(bfhip_ctx *ctx, int n, int P, const double *A, int lda, const double *G, const double *dsc,
                       const double *LinvAll, const int *info, double *h, double *ws, size_t ws_doubles);
// e_loo (n, m) and sums (m, BFHIP_LOO_NSUM) from the residual S (n, m), the weighted targets B (n, m), h and the row weights w
// (n,) or NULL.  Nothing is written when *info != 0.
int bf_loo_sums_launch(bfhip_ctx *ctx, int n, int m, const double *S, const double *B, const double *h, const double *w,
                       const int *info, double *e_loo, double *sums);
