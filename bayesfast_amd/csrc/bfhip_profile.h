// bfhip_profile.h -- one grid line of a profile of the density, as arithmetic for a team of nt threads (bfhip_hess.h has the team's
// rules; tests/profile_host compiles this header for one host thread).
//
// A line holds the coordinates of its mask fixed (bf_newton_run's fixed argument) and moves one of them, walk, through values[0 ..
// n_val - 1].  Every value is one masked maximisation of the objective (BfProfileEval) over the free coordinates, started at the
// optimum of the value before it -- at x_start for the first -- with x[walk] set to the value: a continuation, no tangent predictor.
//   a NaN value ends the line: that column and every later one get NaN and status BF_PROFILE_NOT_RUN
//   a maximisation that ends with status 2 (non-finite) is written as such, and the next value starts from the last optimum whose
//   status was not 2
//   walk < 0 moves nothing: the masked maximisation from x_start, once per column (the entry points ask for n_val == 1)
// The last optimum is read back from the line's own rows of x: element i is written and read by the same thread.
#pragma once
#include "bfhip_hess.h"

#define BF_PROFILE_NOT_RUN 4

// x (n_val, d), logp (n_val), info (n_val, 4) are the line's own rows of the outputs; values may be NULL when walk < 0
template <class Ev>
__host__ __device__ inline void bf_profile_line(Ev &ev, int d, int n_val, int max_iter, double xtol, const uint8_t *fixed, int walk,
                                                const double *x_start, const double *values, double *x, double *logp, double *info,
                                                BfNewtonWork &nw, int tid, int nt) {
    const double *prev = x_start;
    int k = 0;
    for (; k < n_val; ++k) {
        const double v = walk >= 0 ? values[k] : 0.;
        if (v != v) break;
        BF_HESS_SYNC();   // the trial point of the maximisation before is read no more
        for (int i = tid; i < d; i += nt) nw.xt[i] = i == walk ? v : prev[i];
        const BfNewtonStat st = bf_newton_run(ev, d, nw.xt, max_iter, xtol, nw, tid, nt, fixed);   // (copies xt to x behind a barrier)
        double *xk = x + (size_t)k * d;
        for (int i = tid; i < d; i += nt) xk[i] = nw.x[i];
        if (tid == 0) {
            logp[k] = st.logp;
            info[(size_t)k * 4 + 0] = (double)st.n_iter;
            info[(size_t)k * 4 + 1] = (double)st.status;
            info[(size_t)k * 4 + 2] = st.last_step;
            info[(size_t)k * 4 + 3] = st.lam;
        }
        if (st.status != 2) prev = xk;
    }
    const double qnan = nan("");
    for (; k < n_val; ++k) {
        for (int i = tid; i < d; i += nt) x[(size_t)k * d + i] = qnan;
        if (tid == 0) {
            logp[k] = qnan;
            info[(size_t)k * 4 + 0] = 0.;
            info[(size_t)k * 4 + 1] = (double)BF_PROFILE_NOT_RUN;
            info[(size_t)k * 4 + 2] = qnan;
            info[(size_t)k * 4 + 3] = qnan;
        }
    }
}
