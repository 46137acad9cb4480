// bfhip_adapt.h -- the end of a sampler iteration (base_hmc.py:80-85), the ONE copy every sampler kernel evaluates: dual averaging of
// the step size (step_size.py:31-45), one element of the metric's Welford window (metrics.py:354-360), the window logic of
// QuadMetricDiagAdapt.update / QuadMetricFullAdapt.update (metrics.py:186-211, :294-324) and the statistics row.  Host and device
// (tests/test_adapt_host.py sweeps it on the CPU through tests/hess_host; tests/emu compiles it with the group and split kernels).
//
// Everything here works on VALUES: a kernel keeps its scalars where it parks them (LDS slots, registers, the split kernel's cold rows)
// and decides itself which lane stores and what a refresh or a roll does to its vectors or matrices.
//
// ROUNDING.  The adapted step size and the metric are compared bit for bit across kernels, so which operations are fused is decided
// here and nowhere else: every body is under `fp contract(off)`, and the template parameter FUSED says what is written as an fma.
//   FUSED = true   the wave-per-chain family (bf_sampler_kernel, bf_nuts_pipe_kernel, bf_lone_kernel, the Welford update of the
//                  tempered driver): the contractions the compiler chose for that family when it was left to it -- of the two products
//                  of each of dual averaging's sums the one with the NEW term, and the Welford product.
//   FUSED = false  the lane-per-chain family (bf_group_kernel, bf_split_kernel: built with -ffp-contract=off) and its host emulation:
//                  every product rounded on its own, as the reference's NumPy statements are.
// M is a math policy: a type with static ex / lg / sq (exp, log, sqrt; not named so because the sampler translation unit defines
// those names as function-like macros), so that each kernel keeps the form of libm call it needs (out of line, inline behind an
// opaque move, plain).
#pragma once
#include "bfhip_model.h"

// (host and device, always inlined: the convention of bfhip_constraint.h)
#define BF_ADAPT_FN __host__ __device__ inline __attribute__((always_inline))

// what the update needs of `count` alone: 1 / (count + t_0), sqrt(count), count ** -k
struct BfStepConsts {
    double wgt, sq, mk;
};

// DualAverageAdaptation.update while warming up; exp(log_step) and exp(log_bar) are the caller's.  Two ways in, the same operations:
//   step()             the statements in the reference's order, each libm value taken where it is used.  Five kernels call this: where
//                      the libm functions are calls (the sampler translation unit) a value taken early lives across them, and taking
//                      all three ahead of the sums cost bf_nuts_pipe_kernel<4, ...> two to four spilled SGPRs (docs/EXPERIMENTS.md).
//   consts(), update() the three values of `count` alone apart from the rest: the latency kernel takes them early, off its critical path.
template <bool FUSED>
struct BfStepAdapt {
    // (1 - w) x_old + w x_new: the form of both of dual averaging's sums
    static BF_ADAPT_FN double avg(double w, double x_new, double x_old) {
#pragma clang fp contract(off)
        const double keep = (1. - w) * x_old;
        return FUSED ? __builtin_fma(w, x_new, keep) : keep + w * x_new;
    }
    template <class M>
    static BF_ADAPT_FN void step(const bfhip_sampler_config &cfg, double accept_stat, double smu, double &hbar, double &log_step,
                                 double &log_bar, double &count, M) {
#pragma clang fp contract(off)
        hbar = avg(1. / (count + cfg.t_0), cfg.target_accept - accept_stat, hbar);
        log_step = smu - hbar * M::sq(count) / cfg.gamma;
        log_bar = avg(M::ex(-cfg.k * M::lg(count)), log_step, log_bar);   // count ** -k
        count = count + 1.;
    }
    template <class M>
    static BF_ADAPT_FN BfStepConsts consts(const bfhip_sampler_config &cfg, double count, M) {
#pragma clang fp contract(off)
        BfStepConsts c;
        c.wgt = 1. / (count + cfg.t_0);
        c.sq = M::sq(count);
        c.mk = M::ex(-cfg.k * M::lg(count));
        return c;
    }
    static BF_ADAPT_FN void update(const bfhip_sampler_config &cfg, const BfStepConsts &c, double accept_stat, double smu, double &hbar,
                                   double &log_step, double &log_bar, double &count) {
#pragma clang fp contract(off)
        hbar = avg(c.wgt, cfg.target_accept - accept_stat, hbar);
        log_step = smu - hbar * c.sq / cfg.gamma;
        log_bar = avg(c.mk, log_step, log_bar);
        count = count + 1.;
    }
};

// one element of _WeightedVariance.add_sample with weight 1; n is the window's n_samples AFTER its increment
template <bool FUSED>
BF_ADAPT_FN void bf_welford_add(double x, double n, double &mean, double &raw) {
#pragma clang fp contract(off)
    const double od = x - mean;
    mean += od / n;
    raw = FUSED ? __builtin_fma(od, x - mean, raw) : raw + od * (x - mean);
}

// The five scalars of the metric's two windows.  begin(): both windows take the sample (the caller adds it with fg_n and bg_n as they
// are then); refresh(): the metric is to be recomputed from the foreground window (_update_from_weightvar, every update_window
// samples); roll(): the adaptation window is over -- the caller moves its background window to the foreground and empties the
// background, then end() does the same to the counts (an empty window weighs 10: _WeightedVariance's initial_weight) and doubles the
// window.  begin() returns delta, the samples since the last roll, which refresh() and roll() take.  refresh() is a 64-bit remainder, a
// long expansion with branches on the device: it is a call of its own so that it is taken where it is needed, after the Welford
// update -- taken in begin(), ahead of the update, it cost the group and split kernels spills.
struct BfMetricWindow {
    double fg_n, bg_n, n_samples, prev_upd, adapt_window;
    BF_ADAPT_FN long begin() {
        const long delta = (long)(n_samples - prev_upd);
        fg_n += 1.;
        bg_n += 1.;
        return delta;
    }
    static BF_ADAPT_FN bool refresh(const bfhip_sampler_config &cfg, long delta) { return (delta + 1) % (long)cfg.update_window == 0; }
    BF_ADAPT_FN bool roll(long delta) const { return (double)delta >= adapt_window; }
    BF_ADAPT_FN void end(const bfhip_sampler_config &cfg, bool roll) {
        if (roll) {
            fg_n = bg_n;
            bg_n = 10.;
            prev_upd = n_samples;
            if (cfg.doubling) adapt_window *= 2.;
        }
        n_samples += 1.;
    }
};

// the statistics row of one iteration (stats.py:7-14); st points at the row
BF_ADAPT_FN void bf_stats_row_nuts(double *st, double logp, double energy, double depth, double tree_size, double accept_stat,
                                   double step_now, double step_bar, bool warm, double start_energy, double max_de, double diverging) {
    st[BFHIP_NS_LOGP] = logp;
    st[BFHIP_NS_ENERGY] = energy;
    st[BFHIP_NS_TREE_DEPTH] = depth;
    st[BFHIP_NS_TREE_SIZE] = tree_size;
    st[BFHIP_NS_MEAN_TREE_ACCEPT] = accept_stat;
    st[BFHIP_NS_STEP_SIZE] = step_now;
    st[BFHIP_NS_STEP_SIZE_BAR] = step_bar;
    st[BFHIP_NS_WARMUP] = warm ? 1. : 0.;
    st[BFHIP_NS_ENERGY_CHANGE] = energy - start_energy;
    st[BFHIP_NS_MAX_ENERGY_CHANGE] = max_de;
    st[BFHIP_NS_DIVERGING] = diverging;
}
BF_ADAPT_FN void bf_stats_row_hmc(double *st, double logp, double energy, double n_int_step, double accept_stat, double accepted,
                                  double step_now, double step_bar, bool warm, double energy_change, double diverging) {
    st[BFHIP_HS_LOGP] = logp;
    st[BFHIP_HS_ENERGY] = energy;
    st[BFHIP_HS_N_INT_STEP] = n_int_step;
    st[BFHIP_HS_ACCEPT_STAT] = accept_stat;
    st[BFHIP_HS_ACCEPTED] = accepted;
    st[BFHIP_HS_STEP_SIZE] = step_now;
    st[BFHIP_HS_STEP_SIZE_BAR] = step_bar;
    st[BFHIP_HS_WARMUP] = warm ? 1. : 0.;
    st[BFHIP_HS_ENERGY_CHANGE] = energy_change;
    st[BFHIP_HS_DIVERGING] = diverging;
    st[BFHIP_STAT_STRIDE - 1] = 0.;   // (the slot left unused to share the stride with the NUTS row)
}
