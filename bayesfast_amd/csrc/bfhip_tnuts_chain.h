// bfhip_tnuts_chain.h -- the chain driver of the two tempered-NUTS kernels (bfhip_tnuts.hip, bfhip_tnuts_gen.hip): everything a
// chain's wave does between two evaluations of the potentials.  BaseTHMC.astep (samplers/hmc_utils/base_hmc.py:220-262) around the
// NUTS tree (samplers/nuts.py:21-217, TTree: samplers/tnuts.py:15-41) with TCpuLeapfrogIntegrator
// (samplers/hmc_utils/integration.py:98-222): chain state, momentum and v0 draws, the tempered leapfrog step, _build_subtree
// flattened over a per-level stack, Tree.extend with the six-sum U-turn check, dual averaging, the statistics row and the metric's
// adaptation (diagonal Welford windows, or the full-rank covariance with its Cholesky factor: bfhip_metric.h).
//
// A kernel hands in `potentials(q, phi, dphi, psi, dpsi)`, the workgroup's rendezvous around its density.  The driver holds NO
// workgroup barrier of its own and every way out of it (an `err` break, a bad initial energy, i_iter == iter_end) RETURNS to the
// kernel, which goes on answering the rendezvous until no chain of the workgroup is active: every wave passes the same barriers.
// Lane l holds dimensions l E .. l E + E - 1 (E = 2 at the padded dimension DP = 128, 1 below).  Draws are consumed in the recursion's
// post-order, so a chain reproduces the CPU oracle on the same xoshiro stream.
#pragma once
#include <type_traits>
#include "bfhip_sampler_defs.h"
#include "bfhip_wave.h"
#include "bfhip_metric.h"
#include "bfhip_adapt.h"
#include "bfhip_tnuts.h"

// The velocity M^-1 p of a state: kept with the state under the full-rank metric (a matrix-vector product), recomputed as
// var * p under the diagonal one (a product is cheaper than the registers; the same bits either way).
template <int E, bool STORED> struct TnVel { double v[E]; };
template <int E> struct TnVel<E, false> {};

// f(e) for e = 0 .. E - 1, e a compile-time constant: straight-line code, not loops.  At E = 1 a one-trip loop over one-element
// arrays reaches the optimiser's early passes as a loop over memory, and the tuned kernel's W = 4 instantiations with the transform
// or the decay term then spill twelve more registers than with scalars (docs/EXPERIMENTS.md).
template <int E, int I = 0, class F>
__device__ __forceinline__ void tn_each(F &&f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, I>());
        tn_each<E, I + 1>(f);
    }
}

// a . b over a lane's elements.  At E = 1 the product itself (not fma(a, b, 0), which differs in the sign of a zero); at E > 1 the
// sum starts from zero, so that under the library's contraction the terms stay ONE chain of fma in element order -- started from
// the first product, the compiler may fuse either product of a0 b0 + a1 b1 into the other and the bits change.
template <int E>
__device__ inline double tn_dot(const double *a, const double *b) {
    if constexpr (E == 1) {
        return a[0] * b[0];
    } else {
        double r = 0.;
        tn_each<E>([&](auto e) { r += a[e] * b[e]; });
        return r;
    }
}

// The U-turn criterion (nuts.py:56-69, 154-161): one of the N sums a_k . b_k over the dimensions is <= 0 (one reduction).
template <int N, int E>
__device__ inline bool tn_uturn(const double *const (&a)[N], const double *const (&b)[N]) {
    double r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = tn_dot<E>(a[k], b[k]);
    wave_sum_n<N>(r);
    bool turn = false;
#pragma unroll
    for (int k = 0; k < N; ++k) turn = turn || (r[k] <= 0.);
    return turn;
}

// lsw: this wave's [TN_MAXL][TS_N] stack scalars in LDS; matp: this chain's BF_MAT_N matrices (FULLM only)
template <int DP, bool FULLM, class Pot>
__device__ __forceinline__ void tn_run_chain(const TnutsArgs &a, const int chain, const int lane, double *lsw, double *matp, Pot &&potentials) {
    constexpr int E = DP > 64 ? DP / 64 : 1;
    const int d = a.d;
    const size_t msz = (size_t)d * d;
    bool in[E];
    tn_each<E>([&](auto e) { in[e] = lane * E + e < d; });
    // ---- chain state ----
    double *scp = a.sc + (size_t)chain * BFHIP_SC_N;
    double *vecp = a.vec + (size_t)chain * BFHIP_VEC_N * d;
    double *sb = a.scratch + (size_t)chain * (4 * TN_MAXL) * DP + lane * E;
    uint64_t rs[4];
    for (int k = 0; k < 4; ++k) rs[k] = a.rng[(size_t)chain * 4 + k];
    double log_step = scp[BFHIP_SC_LOG_STEP], log_bar = scp[BFHIP_SC_LOG_BAR], hbar = scp[BFHIP_SC_HBAR];
    const double smu = scp[BFHIP_SC_MU];
    double count = scp[BFHIP_SC_COUNT];
    BfMetricWindow mw{scp[BFHIP_SC_FG_N], scp[BFHIP_SC_BG_N], scp[BFHIP_SC_N_SAMPLES], scp[BFHIP_SC_PREV_UPDATE],
                      scp[BFHIP_SC_ADAPT_WINDOW]};
    int i_iter = (int)scp[BFHIP_SC_I_ITER], err = (int)scp[BFHIP_SC_ERROR];
    double qc[E], var[E];
    auto load_vec = [&](int field, double (&v)[E], double pad) {
        tn_each<E>([&](auto e) { v[e] = in[e] ? vecp[field * d + lane * E + e] : pad; });
    };
    auto store_vec = [&](int field, const double (&v)[E]) {
        tn_each<E>([&](auto e) {
            if (in[e]) vecp[field * d + lane * E + e] = v[e];
        });
    };
    load_vec(BFHIP_VEC_Q, qc, 0.);
    load_vec(BFHIP_VEC_VAR, var, 1.);
    double u_cur = rfl(a.tu[chain]);
    unsigned long long nlf = 0;
    auto uni = [&]() { return bf_u01(bf_xoshiro_next(rs)); };
    auto logbern = [&](double l) -> bool {  // nuts.py:200-203
        if (l != l) err = 2;
        return log(uni()) < l;
    };
    // the subtree stack's vector slots: [4 TN_MAXL][DP] per chain
    const bool lane_ok = lane * E < DP;   // (lanes beyond the padded dimension hold zeros and own no slot words)
    auto ldv = [&](int slot, double (&v)[E]) {
        tn_each<E>([&](auto e) { v[e] = lane_ok ? sb[(size_t)slot * DP + e] : 0.; });
    };
    auto stv = [&](int slot, const double (&v)[E]) {
        if (lane_ok) {
            tn_each<E>([&](auto e) { sb[(size_t)slot * DP + e] = v[e]; });
        }
    };
    // velocity of a momentum: metrics.py:88-91 (diagonal), :113-115 (full rank)
    auto vel = [&](const double (&p)[E], double (&out)[E]) {
        if constexpr (FULLM) {
            bf_velocity_full<E>(matp + BF_MAT_COV * msz, p, out, d, lane);
        } else {
            tn_each<E>([&](auto e) { out[e] = var[e] * p[e]; });
        }
    };

    // one tempered leapfrog step from (q, p, u, vt): integration.py:153-222
    // (weight: phi - psi of the state; the importance weight delta / expm1(delta), base_hmc.py:227-231, is taken once per
    // iteration, for the proposal that is kept)
    struct TS : TnVel<E, FULLM> { double q[E], p[E]; double u, vt, weight, energy, logp; };
    auto set_v = [&](TS &s) {   // after a new momentum
        if constexpr (FULLM) vel(s.p, s.v);
    };
    auto get_v = [&](const TS &s, double (&out)[E]) {
        if constexpr (FULLM) {
            tn_each<E>([&](auto e) { out[e] = s.v[e]; });
        } else {
            vel(s.p, out);
        }
    };
    auto finish_state = [&](TS &s, double phi, double psi) {
        double v[E];
        get_v(s, v);
        const double kin = tn_wsum(tn_dot<E>(s.p, v));
        const double ope = 1 + exp(-s.u), beta = 1 / ope, pot = s.u + 2 * log(ope);   // t_beta, t_pot: one exponential
        s.energy = rfl((beta * phi + (1 - beta) * psi + pot) + (0.5 * kin + s.vt * s.vt / 2));
        s.logp = rfl(-phi);
        s.weight = rfl(phi - psi);
    };
    auto t_step = [&](const TS &s0, double eps) -> TS {
        TS s = s0;
        const double dt = 0.5 * eps;
        double phi, dphi[E], psi, dpsi[E], v[E];
        s.u = rfl(s.u + s.vt * dt);
        get_v(s, v);
        tn_each<E>([&](auto e) { s.q[e] += dt * v[e]; });
        potentials(s.q, phi, dphi, psi, dpsi);
        // beta(u) = 1 / (1 + e), beta'(u) = e / (1 + e)^2, U'(u) = (e^u - 1) / (e^u + 1) = (1 - e) / (1 + e) with e = exp(-u): one
        // exponential and one division (the reference's forms to rounding, integration.py:186-200)
        const double ex = exp(-s.u), beta = 1 / (1 + ex), dbeta = ex * beta * beta, dU = (1 - ex) * beta;
        s.vt = rfl(s.vt + -(dbeta * (phi - psi) + dU) * eps);
        tn_each<E>([&](auto e) { s.p[e] += eps * -(beta * dphi[e] + (1 - beta) * dpsi[e]); });
        s.u = rfl(s.u + s.vt * dt);
        set_v(s);
        get_v(s, v);
        tn_each<E>([&](auto e) { s.q[e] += dt * v[e]; });
        potentials(s.q, phi, dphi, psi, dpsi);
        finish_state(s, phi, psi);
        return s;
    };

    while (i_iter < a.iter_end && err == 0) {
        const bool warm = i_iter < a.cfg.n_warmup;
        // ---- BaseTHMC.astep: base_hmc.py:233-262 ----
        TS start;
        {   // p0 = metric.random: one xoshiro draw keys the SplitMix64 stream of the d normals (as in the other kernels)
            const uint64_t K = bf_xoshiro_next(rs);
            tn_each<E>([&](auto e) {
                const int dim = lane * E + e;
                const uint64_t P = (uint64_t)(dim >> 1);
                const double u1 = bf_u01_open0(bf_mix64(K + (2 * P + 1) * BF_GOLDEN)), u2 = bf_u01(bf_mix64(K + (2 * P + 2) * BF_GOLDEN));
                const double rad = sqrt(-2. * log(u1));
                double sn, cs;
                sincospi(2. * u2, &sn, &cs);
                if constexpr (FULLM) start.p[e] = in[e] ? ((dim & 1) ? rad * sn : rad * cs) : 0.;
                else start.p[e] = in[e] ? (1. / sqrt(var[e])) * ((dim & 1) ? rad * sn : rad * cs) : 0.;
                start.q[e] = qc[e];
            });
            if constexpr (FULLM) bf_solve_lt<E>(matp + BF_MAT_CHOL_ROWS * msz, start.p, d, lane);  // metrics.py:123-127
        }
        {   // v0 = rng.normal(0, 1): a stream of its own, first (cosine) element
            const uint64_t K = bf_xoshiro_next(rs);
            const double u1 = bf_u01_open0(bf_mix64(K + BF_GOLDEN)), u2 = bf_u01(bf_mix64(K + 2 * BF_GOLDEN));
            double sn, cs;
            sincospi(2. * u2, &sn, &cs);
            start.vt = rfl(sqrt(-2. * log(u1)) * cs);
        }
        start.u = u_cur;
        set_v(start);
        {
            double phi, dphi[E], psi, dpsi[E];
            potentials(start.q, phi, dphi, psi, dpsi);
            finish_state(start, phi, psi);
        }
        if (!(fabs(start.energy) <= 1.7976931348623157e308)) { err = 1; break; }
        const double eps0 = rfl(exp(warm ? log_step : log_bar));
        // ---- Tree.__init__: nuts.py:24-43 ----
        TS left = start, right = start;
        double prop_q[E], p_sum[E];
        tn_each<E>([&](auto e) { prop_q[e] = start.q[e]; p_sum[e] = start.p[e]; });
        double prop_u = start.u, prop_w = start.weight, prop_E = start.energy, prop_logp = start.logp;
        double log_size = 0., accept_sum = 0., max_de = 0.;
        int depth = 0, n_prop = 0, diverging = 0, turning = 0;
        for (int it = 0; it < a.cfg.max_treedepth && err == 0; ++it) {
            const int dir = logbern(-0.6931471805599453094) ? 1 : -1;  // nuts.py:210
            const double eps = dir > 0 ? eps0 : -eps0;
            const TS old_left = left, old_right = right;
            // ---- _build_subtree(edge, depth, eps), recursion flattened: leaf i merges upwards while bit `lev` of i is set ----
            TS cur = dir > 0 ? right : left;
            // the subtree under construction: first state's momentum (T_lp), last state = cur, p_sum, proposal, log size, accept
            // sum; level 0 of the stack in registers (L0_*)
            double T_lp[E], T_ps[E], T_pq[E], L0_lp[E], L0_rp[E], L0_ps[E], L0_pq[E];
            tn_each<E>([&](auto e) { T_lp[e] = T_ps[e] = T_pq[e] = L0_lp[e] = L0_rp[e] = L0_ps[e] = L0_pq[e] = 0.; });
            double T_pu = 0., T_pw = 0., T_pE = 0., T_plogp = 0., T_ls = 0., T_acc = 0.;
            double sub_acc = 0.;
            long sub_n = 0;
            bool done = false;
            const int n_leaf = 1 << depth;
            for (int i_leaf = 0; i_leaf < n_leaf && !done; ++i_leaf) {
                // ---- _single_step: nuts.py:105-132 ----
                const TS nxt = t_step(cur, eps);
                nlf += 1;
                sub_n += 1;
                double dE = rfl(nxt.energy - start.energy);
                if (dE != dE) dE = INFINITY;
                if (fabs(dE) > fabs(max_de)) max_de = dE;
                if (!(fabs(dE) < a.cfg.max_change)) {
                    diverging = 1;
                    // the stub subtree: ancestors still add their left halves' accept sums (nuts.py:173)
                    for (int al = 0; al < depth; ++al)
                        if ((i_leaf >> al) & 1) sub_acc = rfl(sub_acc + lsw[al * TS_N + TS_ACC]);
                    done = true;
                    break;
                }
                cur = nxt;
                tn_each<E>([&](auto e) { T_lp[e] = nxt.p[e]; T_ps[e] = nxt.p[e]; T_pq[e] = nxt.q[e]; });
                T_pu = nxt.u; T_pw = nxt.weight; T_pE = nxt.energy; T_plogp = nxt.logp;
                T_ls = -dE;
                { const double pa = rfl(exp(-dE)); T_acc = pa > 1. ? 1. : pa; }
                int lev = 0;
                bool abort = false;
                while (lev < depth && ((i_leaf >> lev) & 1)) {
                    // ---- merge with the waiting left sibling of this level: nuts.py:146-178 ----
                    double A_lp[E], A_rp[E], A_ps[E], A_pq[E];  // sibling: left p, right p, p_sum, proposal q
                    if (lev == 0) {
                        tn_each<E>([&](auto e) { A_lp[e] = L0_lp[e]; A_rp[e] = L0_rp[e]; A_ps[e] = L0_ps[e]; A_pq[e] = L0_pq[e]; });
                    } else {
                        ldv(4 * lev + 0, A_lp); ldv(4 * lev + 1, A_rp); ldv(4 * lev + 2, A_ps); ldv(4 * lev + 3, A_pq);
                    }
                    const double *ls = lsw + lev * TS_N;
                    double psum[E], cur_v[E], A_lv[E];
                    tn_each<E>([&](auto e) { psum[e] = A_ps[e] + T_ps[e]; });
                    get_v(cur, cur_v);
                    bool turn;
                    if (lev >= 1) {  // with the sub-span checks for depth > 1 (nuts.py:154-161): six sums, one reduction
                        double A_rv[E], T_lv[E], ps1[E], ps2[E];
                        if constexpr (FULLM) bf_velocity_full3<E>(matp + BF_MAT_COV * msz, A_lp, A_rp, T_lp, A_lv, A_rv, T_lv, d, lane);
                        else { vel(A_lp, A_lv); vel(A_rp, A_rv); vel(T_lp, T_lv); }
                        tn_each<E>([&](auto e) { ps1[e] = A_ps[e] + T_lp[e]; ps2[e] = A_rp[e] + T_ps[e]; });
                        turn = tn_uturn<6, E>({psum, psum, ps1, ps1, ps2, ps2}, {A_lv, cur_v, A_lv, T_lv, A_rv, cur_v});
                    } else {
                        vel(A_lp, A_lv);
                        turn = tn_uturn<2, E>({psum, psum}, {A_lv, cur_v});
                    }
                    const double acc_l = rfl(ls[TS_ACC]), ls_l = rfl(ls[TS_LS]);
                    const double ls_new = rfl(tn_logaddexp(ls_l, T_ls));
                    const bool take2 = logbern(T_ls - ls_new);  // :164 (drawn even when this merge turns)
                    T_acc = rfl(acc_l + T_acc);
                    if (turn) {
                        // the ancestors above still add their accept sums
                        for (int al = lev + 1; al < depth; ++al)
                            if ((i_leaf >> al) & 1) T_acc = rfl(T_acc + lsw[al * TS_N + TS_ACC]);
                        abort = true;
                        turning = 1;
                        break;
                    }
                    if (!take2) {
                        tn_each<E>([&](auto e) { T_pq[e] = A_pq[e]; });
                        T_pE = rfl(ls[TS_E]); T_plogp = rfl(ls[TS_LOGP]); T_pu = rfl(ls[TS_U]); T_pw = rfl(ls[TS_W]);
                    }
                    T_ls = ls_new;
                    tn_each<E>([&](auto e) { T_ps[e] = psum[e]; T_lp[e] = A_lp[e]; });
                    lev += 1;
                }
                if (abort) { sub_acc = T_acc; done = true; break; }
                if (lev < depth) {
                    // wait for the right sibling
                    if (lev == 0) {
                        tn_each<E>([&](auto e) { L0_lp[e] = T_lp[e]; L0_rp[e] = cur.p[e]; L0_ps[e] = T_ps[e]; L0_pq[e] = T_pq[e]; });
                    } else {
                        stv(4 * lev + 0, T_lp); stv(4 * lev + 1, cur.p); stv(4 * lev + 2, T_ps); stv(4 * lev + 3, T_pq);
                    }
                    double *ls = lsw + lev * TS_N;
                    if (lane == 0) { ls[TS_LS] = T_ls; ls[TS_ACC] = T_acc; ls[TS_E] = T_pE; ls[TS_LOGP] = T_plogp; ls[TS_U] = T_pu; ls[TS_W] = T_pw; }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                } else {
                    sub_acc = T_acc;  // the whole subtree of this doubling is complete
                }
            }
            depth += 1;
            accept_sum = rfl(accept_sum + sub_acc);
            n_prop += (int)sub_n;
            if (err) break;
            // Tree.extend returns before touching the ends' p_sum (nuts.py:71-73); the new end replaces the old one only for a
            // complete subtree
            if (diverging || turning) break;
            // ---- Tree.extend after a complete subtree: nuts.py:75-103 ----
            // first and last states of the new subtree: the first leaf (momentum T_lp) follows the old edge, the last one is `cur`
            if (dir > 0) right = cur; else left = cur;
            if (logbern(T_ls - log_size)) {
                tn_each<E>([&](auto e) { prop_q[e] = T_pq[e]; });
                prop_u = T_pu; prop_w = T_pw; prop_E = T_pE; prop_logp = T_plogp;
            }
            log_size = rfl(tn_logaddexp(log_size, T_ls));
            tn_each<E>([&](auto e) { p_sum[e] += T_ps[e]; });  // :86 (in place: the aliases below see the new value)
            {
                // leftmost / rightmost halves: nuts.py:56-69.  An end of a half is state `fwd` when the tree grew forwards and state
                // `bwd` otherwise: its momentum and its velocity
                TS first;   // (momentum and velocity only)
                tn_each<E>([&](auto e) { first.p[e] = T_lp[e]; });
                set_v(first);
                auto end_of = [&](const TS &fwd, const TS &bwd, double (&p)[E], double (&v)[E]) {
                    tn_each<E>([&](auto e) { p[e] = dir > 0 ? fwd.p[e] : bwd.p[e]; });
                    if constexpr (FULLM) {
                        tn_each<E>([&](auto e) { v[e] = dir > 0 ? fwd.v[e] : bwd.v[e]; });
                    } else {
                        vel(p, v);
                    }
                };
                double lm_begin_p[E], lm_begin_v[E], lm_end_p[E], lm_end_v[E], rm_begin_p[E], rm_begin_v[E], rm_end_p[E], rm_end_v[E];
                end_of(old_left, cur, lm_begin_p, lm_begin_v);
                end_of(old_right, first, lm_end_p, lm_end_v);
                end_of(first, old_left, rm_begin_p, rm_begin_v);
                end_of(cur, old_right, rm_end_p, rm_end_v);
                double left_v[E], right_v[E], t1[E], t2[E];
                get_v(left, left_v);
                get_v(right, right_v);
                tn_each<E>([&](auto e) {
                    const double lm_ps = dir > 0 ? p_sum[e] : T_ps[e], rm_ps = dir > 0 ? T_ps[e] : p_sum[e];
                    t1[e] = lm_ps + rm_begin_p[e];
                    t2[e] = lm_end_p[e] + rm_ps;
                });
                turning = tn_uturn<6, E>({p_sum, p_sum, t1, t1, t2, t2}, {left_v, right_v, lm_begin_v, rm_begin_v, lm_end_v, rm_end_v}) ? 1 : 0;
            }
            if (turning) break;
        }
        if (err) break;
        // ---- iteration end: base_hmc.py:252-262 ----
        const double accept_stat = accept_sum / (double)n_prop;
        // step_size.py:31-45.  (This driver's own copy, NOT BfStepAdapt of bfhip_adapt.h: left to the compiler, the tempered kernels' build
        // fuses the product with the OLD term of each sum -- fma(1 - w, hbar, w (target - accept)) --, neither of the helper's forms.)
        if (warm && a.cfg.adapt_step_size) {
            const double wgt = 1. / (count + a.cfg.t_0);
            hbar = ((1. - wgt) * hbar + wgt * (a.cfg.target_accept - accept_stat));
            log_step = smu - hbar * sqrt(count) / a.cfg.gamma;
            const double mk = exp(-a.cfg.k * log(count));
            log_bar = mk * log_step + (1. - mk) * log_bar;
            count += 1.;
        }
        tn_each<E>([&](auto e) { qc[e] = prop_q[e]; });
        u_cur = prop_u;
        const int orow = i_iter - a.iter_out0;
        if (orow >= 0 && orow < a.n_out) {
            if (lane == 0) {
                bf_stats_row_nuts(a.stats + ((size_t)chain * a.n_out + orow) * BFHIP_STAT_STRIDE, prop_logp, prop_E, depth, n_prop, accept_stat,
                                  exp(log_step), exp(log_bar), warm, start.energy, max_de, diverging);
                double *tt = a.stats_t + ((size_t)chain * a.n_out + orow) * 2;
                tt[0] = prop_u;
                tt[1] = (prop_w == 0) ? 1. : prop_w / expm1(prop_w);
            }
            tn_each<E>([&](auto e) {
                if (in[e]) a.samples[((size_t)chain * a.n_out + orow) * d + lane * E + e] = qc[e];
            });
        }
        if (warm && a.cfg.adapt_metric) {
            const long delta = mw.begin();
            const bool roll = mw.roll(delta);
            if constexpr (FULLM) {
                // QuadMetricFullAdapt.update: metrics.py:294-324, _WeightedCovariance.add_sample :401-407 (as in bfhip_sampler.hip)
                double fm[E], bm[E], od[E], nd[E];
                load_vec(BFHIP_VEC_FG_MEAN, fm, 0.);
                load_vec(BFHIP_VEC_BG_MEAN, bm, 0.);
                double *fgT = matp + BF_MAT_FG * msz, *bgT = matp + BF_MAT_BG * msz, *covT = matp + BF_MAT_COV * msz;
                tn_each<E>([&](auto e) { od[e] = qc[e] - fm[e]; fm[e] += od[e] / mw.fg_n; nd[e] = qc[e] - fm[e]; });
                const bool refresh = mw.refresh(a.cfg, delta);   // _update_from_weightvar: :287-292
                bf_welford_cov<E>(fgT, nd, od, d, lane, refresh ? covT : nullptr, mw.fg_n);
                tn_each<E>([&](auto e) { od[e] = qc[e] - bm[e]; bm[e] += od[e] / mw.bg_n; nd[e] = qc[e] - bm[e]; });
                bf_welford_cov<E>(bgT, nd, od, d, lane);
                if (refresh) {
                    double *wT = matp + BF_MAT_WORK * msz;
                    if (bf_chol_rows<E>(covT, wT, d, lane))
                        bf_chol_publish<E>(wT, matp + BF_MAT_CHOL * msz, matp + BF_MAT_CHOL_ROWS * msz, d, lane);
                }
                if (roll) {
                    for (int j = 0; j < d; ++j) {
                        tn_each<E>([&](auto e) {
                            const int i = lane * E + e;
                            if (i < d) {
                                fgT[(size_t)j * d + i] = bgT[(size_t)j * d + i];
                                bgT[(size_t)j * d + i] = (i == j) ? 10. : 0.;  // _WeightedCovariance(n): 10 I
                            }
                        });
                    }
                    tn_each<E>([&](auto e) { fm[e] = bm[e]; bm[e] = 0.; });
                }
                store_vec(BFHIP_VEC_FG_MEAN, fm);
                store_vec(BFHIP_VEC_BG_MEAN, bm);
            } else {
                // QuadMetricDiagAdapt.update: metrics.py:186-211
                double fm[E], fr[E], bm[E], br[E];
                load_vec(BFHIP_VEC_FG_MEAN, fm, 0.); load_vec(BFHIP_VEC_FG_RAW, fr, 0.);
                load_vec(BFHIP_VEC_BG_MEAN, bm, 0.); load_vec(BFHIP_VEC_BG_RAW, br, 0.);
                tn_each<E>([&](auto e) {
                    bf_welford_add<true>(qc[e], mw.fg_n, fm[e], fr[e]);
                    bf_welford_add<true>(qc[e], mw.bg_n, bm[e], br[e]);
                });
                if (mw.refresh(a.cfg, delta)) {
                    tn_each<E>([&](auto e) {
                        if (in[e]) var[e] = fr[e] / mw.fg_n;
                    });
                    store_vec(BFHIP_VEC_VAR, var);
                }
                if (roll) tn_each<E>([&](auto e) { fm[e] = bm[e]; fr[e] = br[e]; bm[e] = 0.; br[e] = 0.; });
                store_vec(BFHIP_VEC_FG_MEAN, fm); store_vec(BFHIP_VEC_FG_RAW, fr);
                store_vec(BFHIP_VEC_BG_MEAN, bm); store_vec(BFHIP_VEC_BG_RAW, br);
            }
            mw.end(a.cfg, roll);
        }
        i_iter += 1;
    }
    // ---- write the chain state back ----
    store_vec(BFHIP_VEC_Q, qc);
    if (lane == 0) {
        for (int k = 0; k < 4; ++k) a.rng[(size_t)chain * 4 + k] = rs[k];
        scp[BFHIP_SC_LOG_STEP] = log_step; scp[BFHIP_SC_LOG_BAR] = log_bar; scp[BFHIP_SC_HBAR] = hbar; scp[BFHIP_SC_COUNT] = count;
        scp[BFHIP_SC_FG_N] = mw.fg_n; scp[BFHIP_SC_BG_N] = mw.bg_n; scp[BFHIP_SC_N_SAMPLES] = mw.n_samples;
        scp[BFHIP_SC_PREV_UPDATE] = mw.prev_upd; scp[BFHIP_SC_ADAPT_WINDOW] = mw.adapt_window;
        scp[BFHIP_SC_I_ITER] = (double)i_iter; scp[BFHIP_SC_ERROR] = (double)err;
        a.tu[chain] = u_cur;
        if (a.n_leapfrog && nlf) atomicAdd(a.n_leapfrog, nlf);
    }
}
