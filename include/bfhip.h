/*
 * bfhip.h -- C ABI of libbfhip.so: the MI355X (gfx950) implementation of BayesFast's data-parallel hot
 * path (polynomial-surrogate logp/grad, leapfrog, NUTS/HMC transitions over many chains, surrogate fit).
 *
 * The reference (h3jia/bayesfast) has no FFI boundary on this path: the seam is Python duck typing
 * (SURVEY.md section 8b).  Each entry point below therefore names the reference *Python/Cython interface*
 * it replaces (file:line relative to the reference root); INTEGRATION.md shows the ctypes binding a
 * maintainer would add on the reference side.
 *
 * Conventions
 *   - plain C, no exceptions: every function returns 0 on success, <0 on error; bfhip_last_error()
 *     returns a message for the calling thread's last failure.
 *   - all array arguments of compute calls are DEVICE pointers owned by the caller (e.g. PyTorch-ROCm
 *     tensor.data_ptr()), row-major float64 unless stated; model descriptions are HOST pointers
 *     and are copied during the upload call.
 *   - one bfhip_ctx per (device, stream); calls on one ctx are not thread-safe, different ctxs are
 *     independent.  Kernels are launched asynchronously on the ctx's stream; nothing synchronises
 *     unless documented.
 */
#ifndef BFHIP_H
#define BFHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bfhip_ctx bfhip_ctx;

#define BFHIP_OK 0
#define BFHIP_ERR_ARG (-1)        /* invalid argument (the reference raises ValueError) */
#define BFHIP_ERR_STATE (-2)      /* bad state, e.g. no density uploaded (RuntimeError) */
#define BFHIP_ERR_HIP (-3)        /* HIP runtime failure */
#define BFHIP_ERR_UNSUPPORTED (-4)/* valid in the reference, not implemented on device yet (NotImplementedError) */

#define BFHIP_MAX_DIM 128         /* input_size limit of the device path */
#define BFHIP_MAX_TREEDEPTH 12

/* bfhip_ridge_path and bfhip_ridge_rotate, the ridge path of the surrogate fit scored by exact leave-one-out for up to 32 penalties in
 * one pass over the rotated design (additions only: the number stays).
 * 116: bfhip_gmm_step (and bfhip_gmm_work_bytes), one EM iteration's pass over the draws for a Gaussian mixture: log density,
 * responsibilities and the weighted moments of every component (additions only).
 * 115: bfhip_health_chains, the per-chain sampler health figures (divergences, tree-depth limit, E-BFMI, depth histogram) read off the
 * statistics table in place (additions only).
 * 114: bfhip_kde_wmean (and bfhip_kde_wmean_work_bytes), the kernel-weighted means over the pairs of bfhip_kde_logsum: the score of the
 * estimate, kernel regression and the mean-shift step (additions only).  bfhip_rw_weights, the smoothed weights of a batch of columns of log
 * ratios written out after the first two bfhip_ploo_* stages, and bfhip_pscale_cjs, the distance between two weighted ECDFs of one
 * parameter for 16 weight columns at once: power-scaling sensitivity (additions only: the number stays).
 * 113: bfhip_kde_logsum (and bfhip_kde_work_bytes), the pairwise log-sum-exp of Gaussian kernels behind the multivariate kernel density
 * estimate and the parameter-shift test (additions only).
 * 112: bfhip_profile_lines and bfhip_pipeline_profile_lines, profiles of the density along grid lines: the device Newton maximiser
 * with coordinates held fixed, walked outward in continuation (additions only).  bfhip_rw_finish (and bfhip_rw_work_bytes), the
 * posterior reweighted to a batch of columns of log ratios after the first two bfhip_ploo_* stages (additions only: the number stays).
 * bfhip_lgo_accum and bfhip_lgo_finish, leave-group-out cross-validation around the same two stages, and bfhip_igamc, the regularised
 * upper incomplete gamma function (additions only: the number stays).
 * 111: bfhip_ploo_moments / _tail / _finish (and bfhip_ploo_work_bytes), pointwise PSIS-LOO and WAIC of a batch of columns of pointwise log
 * likelihoods with a top-M radix select in place of a sort per column (additions only).
 * 110: bfhip_polymodel_columns, a batch of the uploaded polymodel's outputs at draws read in place from the (chain, time, dimension)
 * tensor, and the bound radius of every draw (the posterior predictive summaries).
 * 109: bfhip_lstsq_loo, the leave-one-out validation of the least-squares fit (leverages from the kept factor, held-out residuals,
 * per-output sums).
 * 108: bfhip_marg_quantise / _extent / _hist1d / _index / _hist2d / _levels, the marginal posterior histograms and their credible levels
 * (additions only: the number stays).  bfhip_wave_packs_probe; bfhip_psis and bfhip_wstat_columns / _moments / _cumweights / _quantiles, the Pareto-smoothed importance
 * weights and the weighted posterior table (additions only: the number stays).
 * 107: bfhip_pipeline_logp_hess and bfhip_pipeline_laplace_opt, the analytic and the Gauss-Newton Hessian of the pipeline density and
 * its device Newton maximiser.  106: bfhip_wave_sum_probe.
 * 105: bfhip_diag_columns, bfhip_diag_extent, bfhip_diag_sort and bfhip_diag_rank, the data passes of split-R-hat, ESS and the posterior summary.
 * 104: bfhip_logp_hess and bfhip_laplace_opt, the analytic Hessian of the surrogate density and the device Newton maximiser.
 * 103: bfhip_acor_moments and bfhip_acor_lag_sums, the device integrated autocorrelation time.  102 (round 6): bfhip_polar_ns
 * takes 2 d^2 + n_iter + 10 doubles of work.  101 (round 6): BFHIP_TREE_MODE_WORK grew to 4162 and
 * work[0] of bfhip_tree_size_mode_share carries the laggard bit; 100 before. */
int bfhip_version(void);
const char *bfhip_last_error(void);

/* stream: a hipStream_t (as void*), NULL for the default stream.  device: HIP ordinal. */
int bfhip_ctx_create(bfhip_ctx **out, int device, void *stream);
void bfhip_ctx_destroy(bfhip_ctx *ctx);
int bfhip_ctx_set_stream(bfhip_ctx *ctx, void *stream);
int bfhip_ctx_synchronize(bfhip_ctx *ctx);

/* ------------------------------------------------------------------------------------------------
 * Surrogate density description.  Replaces, as one flattened record, the objects walked per call by
 * Density.logp_and_grad (core/density.py:724-754): the Density's constraint transform
 * (core/density.py:92-140 -> transforms/_constraint.pyx:133-215), the Surrogate input scaling
 * (core/module.py:76-83,226), the PolyModel configs with their masks scattered to full input size
 * (modules/poly.py:466-478, modules/_poly.pyx:13-137), the linear-extrapolation bound
 * (modules/poly.py:480-503) and the decay penalty (core/density.py:740-746).
 * output_size of the surrogate is 1: the surrogate IS the log density -- or, with link_kind = 1, the input m of one
 * downstream analytic module, a Gaussian likelihood logp = link_logp0 - link_prec (m - link_y)^2 / 2, chained as the
 * pipeline does (core/density.py:527-560: the surrogate replaces the modules of its scope, the next module's Jacobian
 * multiplies the surrogate's; e.g. examples/2d-donut.ipynb: m = |x|, logp = -(m - 5)^2 / 0.5).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int d;                        /* input_size, 1..BFHIP_MAX_DIM */
    /* Density.input_scales (d,2) and hard_bounds (d,2) uint8; NULL => identity transform */
    const double *ranges;
    const uint8_t *hard_bounds;   /* may be NULL with ranges set => no hard bound */
    /* Surrogate.input_scales: lower edge (d,) and width (d,); NULL => none */
    const double *su_lo;
    const double *su_diff;
    /* polynomial in surrogate space, masks already scattered to the full input:
     *   f(x) = c0 + lin.x + sum_{j<=k} quad[j,k] x_j x_k + sum_{j,k} cubic2[j,k] x_j^2 x_k
     *          + sum_{j<k<l} cubic3[j,k,l] x_j x_k x_l                                              */
    double c0;
    const double *lin;            /* (d,)   or NULL */
    const double *quad;           /* (d,d)  only j<=k is read (the reference leaves the rest unset) */
    const double *cubic2;         /* (d,d)  or NULL */
    const double *cubic3;         /* (d,d,d) only j<k<l is read, or NULL */
    /* PolyModel bound, modules/poly.py:262-292 */
    int use_bound;
    const double *mu;             /* (d,) */
    const double *hess;           /* (d,d) */
    double alpha;
    double f_mu;
    /* Density decay, core/density.py:761-811.  When decay_mu / decay_hess hold the same numbers as mu / hess bit for bit -- the
     * reference takes both pairs from the fit points by the same statements (modules/poly.py:262-276, core/density.py:796-811) --
     * the decay term's product H_d (x - mu_d) is the bound's H (x - mu) and the kernels run it once. */
    int use_decay;
    const double *decay_mu;       /* (d,) */
    const double *decay_hess;     /* (d,d) */
    double decay_alpha2;
    double decay_gamma;
    /* downstream module of the surrogate's output (see above): 0 none, 1 Gaussian likelihood */
    int link_kind;
    double link_y, link_prec, link_logp0;
} bfhip_density_desc;

/* Copies and re-lays-out the description into device memory (MFMA A-operand fragments). Synchronous. */
int bfhip_density_upload(bfhip_ctx *ctx, const bfhip_density_desc *desc);

/* Density.logp_and_grad(x, original_space, use_surrogate=True) for n points.
 * x (n,d) -> logp (n,), grad (n,d).  Replaces core/density.py:724-754 (which loops rows in Python,
 * core/density.py:523-525).  grad may be NULL. */
int bfhip_logp_grad(bfhip_ctx *ctx, int n, const double *x, int original_space, double *logp, double *grad);

/* Constraint transforms of the uploaded density for n points, x (n,d) -> out (n,d):
 * which = 0 from_original, 1 from_original_grad, 2 from_original_grad2, 3 to_original, 4 to_original_grad,
 * 5 to_original_grad2  (Density.from_original/to_original/..., core/density.py:142-163 ->
 * transforms/_constraint.pyx:19-215; identity / ones / zeros when the density has no input_scales,
 * core/density.py:93-111).  bad (1,) int32 device flag: set to 1+i when variable i of some point is out of
 * bound in a from_original* call (the reference raises ValueError, _constraint.pyx:27-28). */
int bfhip_constraint(bfhip_ctx *ctx, int which, int n, const double *x, double *out, int *bad);

/* CpuLeapfrogIntegrator._step for n chains at once (samplers/hmc_utils/integration.py:68-95) with a
 * diagonal metric (QuadMetricDiag, samplers/hmc_utils/metrics.py:51-91).
 * eps (n,), var (n,d); q,p,grad (n,d) and logp,energy (n,) are updated in place; velocity_out (n,d) may be NULL. */
int bfhip_leapfrog(bfhip_ctx *ctx, int n, const double *eps, const double *var, double *q, double *p,
                   double *grad, double *logp, double *energy, double *velocity_out);

/* ------------------------------------------------------------------------------------------------
 * Sampler.  Per-chain state lives in caller-owned device arrays so that a later run() continues the
 * chains (SURVEY.md section 5 "checkpoint/resume"; samplers/hmc_utils/base_hmc.py:98-111).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    /* _HTrace / NTrace / HTrace hyper-parameters, samplers/sample_trace.py:159-172,460-512 */
    int sampler;                  /* 0 = NUTS (samplers/nuts.py), 1 = HMC (samplers/hmc.py) */
    int n_warmup;
    int max_treedepth;            /* NUTS, <= BFHIP_MAX_TREEDEPTH */
    int n_int_step;               /* HMC */
    double max_change;
    double target_accept, gamma, k, t_0;
    int adapt_step_size;
    int adapt_metric;
    int update_window;
    int doubling;
    /* Full-rank metric, QuadMetricFull / QuadMetricFullAdapt (samplers/hmc_utils/metrics.py:94-132,240-330).
     * 0 / NULL: the diagonal metric of `vec`.  Otherwise metric_mat points to the per-chain matrices filled by
     * bfhip_metric_init_full, (n_chain, BFHIP_MAT_N, d, d) doubles on the device; adapt_metric chooses between the
     * fixed (QuadMetricFull) and the adaptive (QuadMetricFullAdapt) variant exactly as for the diagonal metric. */
    int full_metric;
    double *metric_mat;
    /* How the chains of a 16-chain workgroup are laid out (common surrogate at d <= 64, diagonal metric; ignored elsewhere).
     * 1 = lane per chain (bfhip_group.hip): one instruction advances the scalar logic of all 16 chains; fastest while the
     *     chains of a workgroup stay in step (every tree the same size), slow when they do not, because every trip then
     *     executes the union of the chains' paths.
     * 2 = wave per chain (bfhip_sampler.hip: pipelined / sliced kernels): each chain follows its own path; insensitive to
     *     chains out of step.
     * 3 = "split": the lane-per-chain layout with eight waves per 16 chains, two per SIMD with disjoint work -- integrator
     *     waves (leapfrog step, gradient tiles) and bookkeeper waves (the NUTS tree, one leaf behind); NUTS on the plain
     *     common surrogate at 33 <= d <= 64, anything else runs as 1.  Bit-identical results to 1.
     * 0 = library default: 2 for NUTS, 1 for HMC (whose chains are always in step).  bayesfast_amd.chains.DeviceChains
     *     chooses 1 / 3 or 2 per run from the tree sizes of the previous run. */
    int chain_layout;
} bfhip_sampler_config;

/* matrices per chain for the full-rank metric (layout documented in bayesfast_amd/csrc/bfhip_metric.h; slot
 * BFHIP_MAT_COV holds the covariance transposed, i.e. as is for a symmetric matrix) */
#define BFHIP_MAT_COV 0
#define BFHIP_MAT_N 6

/* Layout of the per-chain scalar state array `sc` (C, BFHIP_SC_N) float64 */
enum {
    BFHIP_SC_LOG_STEP = 0,   /* DualAverageAdaptation._log_step, samplers/hmc_utils/step_size.py:13 */
    BFHIP_SC_LOG_BAR,        /* _log_bar */
    BFHIP_SC_HBAR,           /* _hbar */
    BFHIP_SC_MU,             /* _mu = log(10 * initial_step) */
    BFHIP_SC_COUNT,          /* _count */
    BFHIP_SC_FG_N,           /* _WeightedVariance.n_samples of the foreground window, metrics.py:337 */
    BFHIP_SC_BG_N,           /* same, background window */
    BFHIP_SC_N_SAMPLES,      /* QuadMetricDiagAdapt._n_samples */
    BFHIP_SC_PREV_UPDATE,    /* _previous_update */
    BFHIP_SC_ADAPT_WINDOW,   /* _adapt_window (doubles when `doubling`) */
    BFHIP_SC_I_ITER,         /* iterations done (len(trace._samples)) */
    BFHIP_SC_ERROR,          /* 0 ok; 1 bad initial energy (base_hmc.py:72-76); 2 logbern(NaN) (nuts.py:201-202); 3 metric covariance not positive definite (metrics.py:107-108) */
    BFHIP_SC_N
};

/* Layout of the per-chain vector state array `vec` (C, BFHIP_VEC_N, d) float64 */
enum {
    BFHIP_VEC_Q = 0,         /* current position: last sample, or x_0 (transformed space) */
    BFHIP_VEC_VAR,           /* QuadMetricDiag._var */
    BFHIP_VEC_FG_MEAN, BFHIP_VEC_FG_RAW, BFHIP_VEC_BG_MEAN, BFHIP_VEC_BG_RAW, /* metrics.py:333-371 */
    BFHIP_VEC_N
};

/* NUTS statistics per iteration, order of samplers/hmc_utils/stats.py:12-14 */
enum {
    BFHIP_NS_LOGP = 0, BFHIP_NS_ENERGY, BFHIP_NS_TREE_DEPTH, BFHIP_NS_TREE_SIZE, BFHIP_NS_MEAN_TREE_ACCEPT,
    BFHIP_NS_STEP_SIZE, BFHIP_NS_STEP_SIZE_BAR, BFHIP_NS_WARMUP, BFHIP_NS_ENERGY_CHANGE,
    BFHIP_NS_MAX_ENERGY_CHANGE, BFHIP_NS_DIVERGING, BFHIP_NS_N
};
/* HMC statistics, order of samplers/hmc_utils/stats.py:7-9 (one slot left unused to share the stride) */
enum {
    BFHIP_HS_LOGP = 0, BFHIP_HS_ENERGY, BFHIP_HS_N_INT_STEP, BFHIP_HS_ACCEPT_STAT, BFHIP_HS_ACCEPTED,
    BFHIP_HS_STEP_SIZE, BFHIP_HS_STEP_SIZE_BAR, BFHIP_HS_WARMUP, BFHIP_HS_ENERGY_CHANGE, BFHIP_HS_DIVERGING,
    BFHIP_HS_N
};
#define BFHIP_STAT_STRIDE 11

/* Runs every chain from its own i_iter up to (excluding) iter_end: BaseHMC.run/astep
 * (samplers/hmc_utils/base_hmc.py:62-85,155-156) with NUTS._hamiltonian_step (samplers/nuts.py:205-217,
 * Tree :21-189) or HMC._hamiltonian_step (samplers/hmc.py:16-49), for n_chain chains in one launch.
 *   rng     (C,4) uint64  per-chain xoshiro256++ state (bfhip_rng_seed)
 *   sc      (C,BFHIP_SC_N) float64, vec (C,BFHIP_VEC_N,d) float64: state above, updated in place
 *   samples (C,n_out,d): iteration i of a chain is written to row i - iter_out0
 *   stats   (C,n_out,BFHIP_STAT_STRIDE)
 *   n_leapfrog (1,) uint64 device counter, incremented by the number of leapfrog steps taken (may be NULL)
 * Asynchronous. */
int bfhip_sampler_run(bfhip_ctx *ctx, const bfhip_sampler_config *cfg, int n_chain, int iter_end,
                      uint64_t *rng, double *sc, double *vec, int iter_out0, int n_out, double *samples,
                      double *stats, unsigned long long *n_leapfrog);

/* Helper of the layout choice (chain_layout above): work[0] := the most common tree_size (1 .. 4095; larger sizes count as 4095)
 * when at least `share` of the NUTS trees in rows [row0, row0 + n_rows) of stats (C,n_out,BFHIP_STAT_STRIDE), all chains, have it,
 * else 0; plus 4096 -- whether or not the trees are in step -- when some chain's trees of these rows add up to at least four times
 * the mean over the chains (to the resolution of the size classes 1, 2, 3, 4, 6, 8, 12, ...: a launch lasts as long as its busiest
 * chain).  Read it as (work[0] & 4095, work[0] >> 12).
 * work: BFHIP_TREE_MODE_WORK int32 on the device, zeroed once by the caller and left clean by every call (the kernel writes all
 * BFHIP_TREE_MODE_WORK entries: a binding built against bfhip_version() 100, where the buffer was 4098 ints, must be rebuilt).
 * Queued on the context's stream behind the launch that wrote the rows; nothing synchronises. */
#define BFHIP_TREE_MODE_WORK 4162
int bfhip_tree_size_mode_share(bfhip_ctx *ctx, int n_chain, int n_out, const double *stats, int row0, int n_rows, double share,
                               int *work);

/* ------------------------------------------------------------------------------------------------
 * Tempered NUTS: TNUTS (samplers/tnuts.py:15-41) = BaseTHMC.astep
 * (samplers/hmc_utils/base_hmc.py:220-262) + the NUTS tree + TCpuLeapfrogIntegrator (samplers/hmc_utils/integration.py:98-222).
 * The target is the uploaded surrogate density (common surrogate: linear + quadratic configs with the bound, optionally behind the
 * constraint transform -- input_scales / hard bounds -- and with the decay term; surrogate input scales fold away at upload;
 * d <= 64, diagonal metric); the base density of TNTrace(density_base=..., logxi=...) (samplers/sample_trace.py:540-567,607-629) is a
 * quadratic log-density  c0 + lin.x + x.S x / 2  given by DEVICE arrays (e.g. a Gaussian).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const double *base_S;    /* (d,d) symmetric, device */
    const double *base_lin;  /* (d,), device */
    double base_c0;
    double logxi;            /* _TTrace.logxi */
} bfhip_tempering;

/* As bfhip_sampler_run (sampler = NUTS), plus: u (C,) the tempering coordinate of every chain (in: u_0 -- the reference draws
 * it from numpy's global generator, base_hmc.py:241 --, out: u of the last sample); stats_t (C,n_out,2) = (u, weight) of every
 * sample (TNStepStats, samplers/hmc_utils/stats.py).  One normal draw more per iteration than NUTS (v_0, base_hmc.py:245).
 * THMC is not offered: the reference's THTrace constructor raises (samplers/sample_trace.py:600). */
int bfhip_tnuts_run(bfhip_ctx *ctx, const bfhip_sampler_config *cfg, const bfhip_tempering *tp, int n_chain, int iter_end,
                    uint64_t *rng, double *sc, double *vec, double *u, int iter_out0, int n_out, double *samples, double *stats,
                    double *stats_t, unsigned long long *n_leapfrog);

/* Fills rng (C,4) with xoshiro256++ states for streams first_stream .. first_stream+C-1 of `seed`
 * (counterpart of utils/random.py:20-32 spawn_generator: one independent stream per GLOBAL chain index). */
int bfhip_rng_seed(bfhip_ctx *ctx, int n_chain, uint64_t seed, uint64_t first_stream, uint64_t *rng);

/* Initialises sc/vec for fresh chains: _HTrace._init_chain (samplers/sample_trace.py:178-202),
 * _set_step_size_2 (:365-373) and _set_metric_2 (:424-455).
 * x0 (C,d); metric_var (d,) or NULL (ones); initial_mean (d,) or NULL (x0 of each chain). */
int bfhip_chain_init(bfhip_ctx *ctx, int n_chain, int d, const double *x0, double step_size,
                     const double *metric_var, const double *initial_mean, double initial_weight,
                     int adapt_window, double *sc, double *vec);

/* Full-rank metric for fresh chains: _set_metric_2 with a 2-d metric (samplers/sample_trace.py:424-455),
 * QuadMetricFull.__init__ / QuadMetricFullAdapt.__init__ (metrics.py:103-111,261-285).
 * cov0 (d,d) row-major or NULL (identity), shared by all chains; mat (C, BFHIP_MAT_N, d, d).  Call after
 * bfhip_chain_init (the Welford means and weights live in sc/vec).  A cov0 that is not positive definite sets
 * sc[:, BFHIP_SC_ERROR] = 3 for every chain (the reference raises ValueError, metrics.py:107-108). */
int bfhip_metric_init_full(bfhip_ctx *ctx, int n_chain, int d, const double *cov0, double initial_weight,
                           double *sc, double *mat);

/* ------------------------------------------------------------------------------------------------
 * Multi-output surrogate module: PolyModel.fun / jac / fun_and_jac for output_size m > 1
 * (modules/poly.py:430-503).  Linear, quadratic and cubic configs, masks already scattered by
 * the caller: c0 (m), lin (m,d), quad (m,d,d) with the upper triangle j <= k as in bfhip_density_desc.
 * The extrapolation bound (mu, hess, alpha) is shared by all outputs, f_mu (m) is per output.
 * ---------------------------------------------------------------------------------------------- */
typedef struct bfhip_polymodel_desc {
    int d, m;
    const double *c0, *lin, *quad;  /* quad may be NULL (all-linear model) */
    int use_bound;
    const double *mu, *hess;        /* (d), (d,d) */
    double alpha;
    const double *f_mu;             /* (m) */
    /* cubic configs (modules/_poly.pyx:49-137), compact over the dimensions they touch: mask2 (n2,) / mask3 (n3,) sorted
     * dimension indices; cubic2 (m, n2, n2): f_o += sum_{j,k} cubic2[o,j,k] x_j^2 x_k; cubic3 (m, n3, n3, n3), only
     * j < k < l is read: f_o += sum_{j<k<l} cubic3[o,j,k,l] x_j x_k x_l (x restricted to the mask).  NULL / 0: none. */
    int n2;
    const int *mask2;
    const double *cubic2;
    int n3;
    const int *mask3;
    const double *cubic3;
} bfhip_polymodel_desc;

/* Copies the module into device memory owned by the context (host pointers in the descriptor). */
int bfhip_polymodel_upload(bfhip_ctx *ctx, const bfhip_polymodel_desc *desc);

/* f (n,m) and, if jac != NULL, jac (n,m,d) for n points x (n,d); device pointers.  Outside the bound every output
 * is extrapolated linearly from the projected point, PolyModel._fj_bound (modules/poly.py:480-503). */
int bfhip_polymodel_eval(bfhip_ctx *ctx, int n, const double *x, double *f, double *jac);

/* Outputs k0 .. k0 + nb - 1 of the uploaded polymodel at draws read in place from the time-major sample tensor (no Jacobian):
 *   point (c, i), c < n_chain, i < n_draw, has the coordinates x[c ldw + (since + i) ldr + j], j < d -- the addressing of
 *   bfhip_diag_columns (float64, or float32 read as float64 when is_f32; ldr >= d); n = n_chain n_draw <= 2^31 - 1;
 *   in_lo, in_diff (d) device pointers, both or neither: the model sees xs_j = (x_j - in_lo[j]) / in_diff[j], that subtraction and
 *   that division in float64;
 *   out[(c n_draw + i) ldo + b] = output k0 + b at xs as bfhip_polymodel_eval defines it (every config order, the bound test, the
 *   linear extrapolation from the projected point), b < nb, 1 <= nb, k0 + nb <= m, ldo >= nb; columns nb .. ldo - 1 are not written;
 *   beta (n) or NULL: beta[c n_draw + i] = sqrt((xs - mu)^T H (xs - mu)) of the uploaded bound, 0 when the model carries none (an
 *   all-linear model ignores its bound); a point is outside exactly when beta > alpha.
 * A value depends on its point and its output only: not on k0, nb, ldo, n_chain, the size of the launch or the point's place in its
 * 16-point tile.  Stream-ordered, no host synchronisation.  BFHIP_ERR_STATE without an uploaded polymodel, BFHIP_ERR_UNSUPPORTED for
 * n > 2^31 - 1; n_chain = 0 or n_draw = 0 returns 0 without a launch; a refused call leaves the uploaded model usable. */
int bfhip_polymodel_columns(bfhip_ctx *ctx, int n_chain, long n_draw, long ldw, long ldr, const void *x, int is_f32, long since,
                            const double *in_lo, const double *in_diff, int k0, int nb, double *out, long ldo, double *beta);

/* Downstream analytic module of a pipeline whose first module is the multi-output surrogate: a Gaussian likelihood
 * (chi-square) of its m outputs, with the pipeline's chain rule (core/density.py:552-560: jac = dot(J_out, J_in)) fused in:
 *   r = prec (f - y)  (prec (m,m) row-major, or prec_diag (m) when prec is NULL),  logp = -1/2 (f - y).r + logp0,
 *   grad = -J^T r,  J (n,m,d) the surrogate's Jacobians.
 * f (n,m), jac (n,m,d) as written by bfhip_polymodel_eval; logp (n), grad (n,d); grad may be NULL. */
int bfhip_chi2_stage(bfhip_ctx *ctx, int n, int m, int d, const double *f, const double *jac, const double *y, const double *prec,
                     const double *prec_diag, double logp0, double *logp, double *grad);

/* ------------------------------------------------------------------------------------------------
 * Pipeline density: the density of a Density whose module list is
 *   [model (replaced by a multi-output PolyModel surrogate), Gaussian likelihood of its m outputs, optional prior module]
 * with use_surrogate=True -- core/density.py:487-566 (the surrogate replaces the modules of its scope, :527-551; every
 * later module's Jacobian multiplies the ones before it, :552-560), modules/poly.py:430-503 (multi-output evaluation and
 * the bound's linear extrapolation), core/density.py:724-754 (transform, decay); the shape of
 * examples/des-y1-w-cosmosis.ipynb cells 12-18 (d = 27, m = 457: chi2_f / chi2_fj on the whitened data vector, des_post_f /
 * des_post_fj adding a Gaussian prior of some inputs).
 *   like  = logp0 - (f(x) - y)^T prec (f(x) - y) / 2          prec (m,m) symmetric positive definite, or diag(prec_diag)
 *   logp  = like + prior_c0 - sum_i prior_prec[i] (x_i - prior_mu[i])^2 / 2        (prior_*: original-space inputs; optional)
 * After the upload this IS the context's density: bfhip_logp_grad, bfhip_constraint and bfhip_sampler_run (NUTS / HMC,
 * diagonal metric, d <= 64) run on it.  The (m, d) Jacobian is never formed: the Cholesky factor of prec is folded into
 * the coefficient matrix at upload and grad = -(d phi / dx)^T C'^T (C' phi - y') is two FP64-MFMA contractions per
 * evaluation with the 16 chains of a workgroup as columns (bayesfast_amd/csrc/bfhip_pld.h).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int d, m;
    const double *ranges;         /* as bfhip_density_desc */
    const uint8_t *hard_bounds;
    const double *su_lo, *su_diff;
    bfhip_polymodel_desc model;   /* the surrogate: dense per-output coefficients, masks scattered; model.d = d, model.m = m */
    const double *y;              /* (m) */
    const double *prec;           /* (m,m) row-major, or NULL */
    const double *prec_diag;      /* (m) when prec is NULL */
    double logp0;
    const double *prior_mu;       /* (d) or NULL */
    const double *prior_prec;     /* (d) inverse variances, 0 where an input has no prior; NULL with prior_mu */
    double prior_c0;
    int use_decay;                /* as bfhip_density_desc */
    const double *decay_mu, *decay_hess;
    double decay_alpha2, decay_gamma;
} bfhip_pipeline_desc;

/* Copies, whitens and re-lays-out the description into device memory.  Synchronous.  BFHIP_ERR_ARG when prec is not positive
 * definite; BFHIP_ERR_UNSUPPORTED when d > 64 or the working set of one workgroup does not fit the CU's LDS. */
int bfhip_pipeline_upload(bfhip_ctx *ctx, const bfhip_pipeline_desc *desc);

/* ------------------------------------------------------------------------------------------------
 * Surrogate fit, PolyModel.fit (modules/poly.py:505-589).
 * ---------------------------------------------------------------------------------------------- */
/* Design-matrix block for one PolyConfig: x (n, n_in) gathered inputs -> A[:, col0 : col0+width] of the
 * row-major (n, lda) matrix A.  order: 0 linear (1 | x), 1 quadratic, 2 cubic-2, 3 cubic-3.
 * Replaces modules/poly.py:537-564 -> modules/_poly.pyx:143-177.  Optional row weights w (n,) scale the
 * block (modules/poly.py:566-568). */
int bfhip_design_block(bfhip_ctx *ctx, int order, int n, int n_in, const double *x, const double *w,
                       double *A, int lda, int col0);

/* Normal equations with FP64 MFMA: G (P,P) = A^T A, r (P,m) = A^T B for A (n,P), B (n,m), row-major.
 * Stands in for the factorisation inside scipy.linalg.lstsq (modules/poly.py:570). */
int bfhip_gram(bfhip_ctx *ctx, int n, int P, int m, const double *A, int lda, const double *B, double *G, double *r);

/* Solves G c = r for SPD G (P,P) in place by blocked Cholesky on device: r (P,m) is overwritten by the solution, G by
 * the factor of the Jacobi-equilibrated matrix in the solver's own layout (64 x 64 diagonal blocks of L in place, the
 * blocks below the diagonal TRANSPOSED in the upper triangle; the strict lower triangle holds work values).  info (1,)
 * int32 device flag: 0 ok, k>0 pivot k of the equilibrated matrix below 1e-11 (1-based, the first one). */
int bfhip_solve_spd(bfhip_ctx *ctx, int P, int m, double *G, double *r, int *info);

/* The least-squares solve of PolyModel.fit in one call (scipy.linalg.lstsq(A, b), modules/poly.py:570): c (P,m) =
 * argmin |A c - B| for A (n,lda>=P), B (n,m), by the normal equations above followed by n_refine steps of refinement on
 * the true residual, c += G^-1 A^T (B - A c), with the kept Cholesky factor (corrected semi-normal equations: the
 * coefficient error drops from cond(A)^2 eps to the cond(A) eps of an orthogonal factorisation).  G (P,P) receives the
 * factor; work holds n*m + P*m doubles (may be NULL when n_refine = 0).  info as in bfhip_solve_spd: a pivot of the
 * equilibrated matrix below 1e-11 is reported as rank deficiency and c is then not meaningful -- the caller
 * regularises, it is never silent.  Checked against the reference's gelsd up to a column-equilibrated cond(A) of 1e7
 * (two steps: 1e-10 of the coefficient scale, tests/golden/fit_illcond.npz). */
int bfhip_lstsq(bfhip_ctx *ctx, int n, int P, int m, const double *A, int lda, const double *B, double *G, double *c,
                int n_refine, double *work, int *info);

/* bfhip_lstsq with the leave-one-out validation of the fit it has just made (PolyModel.fit_loo).  For linear least squares the
 * residual of row i under a fit without row i is S_i / (1 - h_i) exactly, h_i = a_i^T (A^T A)^-1 a_i = | L^-1 D a_i |^2 the
 * leverage of design row a_i: no refit, n P^2 operations with the kept factor, on the FP64 matrix cores.  The first twelve
 * arguments, c, G and info are bfhip_lstsq's (the same launches, the same bits); after the refinement
 *   h (n,)        the leverages;
 *   e_loo (n, m)  S / ((1 - h) w), S = B - A c at the returned c: the held-out residuals in the units of B / w (w (n,) are the
 *                 row weights A and B were built with, NULL for none).  A row with 1 - h <= 0 after rounding gets +-inf;
 *   sums (m, BFHIP_LOO_NSUM)  per output, summed over the rows in a fixed order, in the units of B (the weighted ones):
 *                 [BFHIP_LOO_SSE] sum S^2, [_PRESS] sum (S / (1 - h))^2, [_MAX] max |e_loo| and [_ARGMAX] its (first) row,
 *                 [_SY] sum B, [_SYY] sum B^2, [_NUNIT] the number of rows with 1 - h <= 0 (their infinities are in _PRESS and
 *                 _MAX too), [7] zero.
 * h, e_loo and sums are given together or all NULL; all NULL is bfhip_lstsq exactly (w, ws unused, nothing more is launched).
 * Otherwise work (n m + P m doubles) is needed whatever n_refine, and ws, a workspace of ws_doubles doubles: a workgroup takes
 * BFHIP_LOO_TILE design rows through the factor and keeps its part of L^-1 D a in a slice of ceil(P / 64) * 64 * BFHIP_LOO_TILE
 * doubles, so the workspace holds ws_doubles / slice tiles side by side and the rows are taken in as many passes as that asks
 * for (BFHIP_ERR_ARG if it holds none).  No more than BFHIP_LOO_WS_MAX doubles (2 GiB) of it are used.  Two calls give the same
 * bits, whatever the workspace's size.  info != 0 (rank deficiency): h, e_loo and sums are left untouched. */
#define BFHIP_LOO_TILE 64
#define BFHIP_LOO_WS_MAX (1L << 28)
#define BFHIP_LOO_NSUM 8
#define BFHIP_LOO_SSE 0
#define BFHIP_LOO_PRESS 1
#define BFHIP_LOO_MAX 2
#define BFHIP_LOO_ARGMAX 3
#define BFHIP_LOO_SY 4
#define BFHIP_LOO_SYY 5
#define BFHIP_LOO_NUNIT 6
int bfhip_lstsq_loo(bfhip_ctx *ctx, int n, int P, int m, const double *A, int lda, const double *B, double *G, double *c,
                    int n_refine, double *work, int *info, double *h, double *e_loo, double *sums, const double *w, double *ws,
                    size_t ws_doubles);

/* The ridge path of the fit scored by exact leave-one-out (PolyModel.fit_ridge).  For a fixed penalty ridge regression is least
 * squares on augmented data, so S_i / (1 - h_i(lam)) is still the residual of row i under a fit without it.  The caller brings ONE
 * symmetric eigen-decomposition: eigenvalues Lam (r,) >= 0, the rows of the rotated design Z (n, ldz >= r) and T (r, m) = Z^T B';
 * the call scores all L <= BFHIP_RIDGE_MAX_L penalties lambdas (L,) > 0 (device arrays, like every array here) in one pass over Z,
 * on the FP64 matrix cores, the right operand T_jo g_jl made as it is used:
 *   complement = 0:  h_il = h0_i + sum_j z_ij^2 g_jl,  S_iol = B'_io - sum_j z_ij T_jo g_jl,  g_jl = 1 / (Lam_j + lambda_l);
 *   complement = 1 (more columns than rows; Z orthonormal columns that span what h0 leaves, Lam and T in that basis):
 *                    1 - h_il = sum_j z_ij^2 g_jl,  S_iol = sum_j z_ij T_jo g_jl,  g_jl = lambda_l / (Lam_j + lambda_l), summed
 *                    directly: nothing of the form 1 - (...) cancels.  Bp and h0 are not read.
 * Bp (n, m) are the targets B' the fit sees, Bw (n, m) the weighted targets of the SY / SYY slots, h0 (n,) the leverage of the
 * unpenalised part or NULL, w (n,) the row weights or NULL.
 *   h (n, L)                      the leverages;
 *   sums (L, m, BFHIP_LOO_NSUM)   per penalty and output, the slots of bfhip_lstsq_loo with the same definitions (e_loo =
 *                                 S / ((1 - h) w); +-inf and a count in _NUNIT where 1 - h <= 0; _ARGMAX the first row of the maximum);
 *   resid, e_loo (n, m)           S / w and e_loo, both in the units of B / w: given together or both NULL, and only for L = 1.
 * row0: the rows are rows row0 .. row0 + n - 1 of a longer series taken in passes (a multiple of BFHIP_RIDGE_TILE): _ARGMAX counts
 * from it and, when row0 > 0, the sums continue those already in `sums`, in the order one call over all rows has.  work holds
 * BFHIP_RIDGE_WORK(n, r, m, L) doubles.  The order of every sum is fixed by (n, r, m, L): two calls give the same bits, and so do passes. */
#define BFHIP_RIDGE_MAX_L 32
#define BFHIP_RIDGE_TILE 64
#define BFHIP_RIDGE_WORK(n, r, m, L) \
    ((size_t)(r) * BFHIP_RIDGE_MAX_L + (size_t)(((n) + BFHIP_RIDGE_TILE - 1) / BFHIP_RIDGE_TILE) * (size_t)(L) * (size_t)(m) * 7)
int bfhip_ridge_path(bfhip_ctx *ctx, int n, int r, int m, int L, const double *Z, int ldz, const double *Lam, const double *T,
                     const double *lambdas, const double *Bp, const double *Bw, const double *h0, const double *w, int complement,
                     long row0, double *h, double *sums, double *resid, double *e_loo, double *work, size_t work_doubles);
/* Z (n, ldz >= r) = A (n, lda >= P) V (P, ldv >= r), row-major, on the FP64 matrix cores: the rows of a design in the eigenbasis.
 * A row's sums run over the columns of A in order whatever n is, so rows rotated in passes have the bits of one call. */
int bfhip_ridge_rotate(bfhip_ctx *ctx, int n, int P, int r, const double *A, int lda, const double *V, int ldv, double *Z, int ldz);

/* ------------------------------------------------------------------------------------------------
 * Refit glue: the steps either side of the sampler inside Recipe._sam_step / _pos_step.
 * ---------------------------------------------------------------------------------------------- */
/* Stable ascending sort of a (n,) float64 by value, every NaN last (the order of np.argsort(a), utils/misc.py:108, with
 * ties kept in index order): keys_sorted (n,) uint64 order-preserving keys, order (n,) int64 the permutation.
 * SystematicResampler.run(a, m) is order[ranks] for the m ranks of its index pattern (utils/misc.py:92-100). */
int bfhip_sort_keys(bfhip_ctx *ctx, long n, const double *a, uint64_t *keys_sorted, int64_t *order);

/* keys (n,) uint64 of a (n,) float64, unsorted (the same mapping as bfhip_sort_keys). */
int bfhip_order_keys(bfhip_ctx *ctx, long n, const double *a, uint64_t *keys);

/* For a sorted shard keys_sorted (n,): counts[i] = number of keys < q[i] (upper = 0) or <= q[i] (upper = 1), q (nq,).
 * The sharded form of the rank selection: ranks that share no data-path collective bisect on the key values and
 * all-reduce these counts (bayesfast_amd/core/refit.py; SURVEY section 8e option ii). */
int bfhip_count_keys(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, long nq, const uint64_t *q, int upper, int64_t *counts);

/* PostStep's importance weights (core/recipe.py:1289-1296): w = exp(logp - logq), w_trunc = clip(w, 0, mean(w) n^k_trunc)
 * (w_trunc = w for k_trunc < 0) with np.clip's NaN semantics: one NaN weight makes every w_trunc NaN; all arrays (n,) float64
 * on the device. */
int bfhip_importance_weights(bfhip_ctx *ctx, long n, const double *logp, const double *logq, double k_trunc, double *w,
                             double *w_trunc);

/* ------------------------------------------------------------------------------------------------
 * Evidence: Gaussianized bridge sampling = SIT + bridge.
 * ---------------------------------------------------------------------------------------------- */
/* kde.cdf (utils/kde.py:322-354) of d one-dimensional weighted Gaussian KDEs at m points each:
 * out[j][i] = sum_k w[k] ndtr((pts[j][i] - data[j][k]) / h[j]).  data (d,n), w (n) normalised, h (d) bandwidths,
 * pts (d,m), out (d,m).  SIT._gaussianize_1d (transforms/sit.py:223-227) applies norm.ppf to it at the spline knots. */
int bfhip_kde_cdf(bfhip_ctx *ctx, int d, long n, const double *data, const double *w, const double *h, int m, const double *pts,
                  double *out);

/* The pairwise sum of a multivariate Gaussian kernel density estimate (utils/kde.py:265-320 of the reference, its pdf and logpdf
 * without the d x d whitening and the normalisation, which stay with the caller):
 *     out[i] = log sum_j exp(logw[j] - |zq_i - z_j|^2 / 2),   i < m, j < n,
 * a true log-sum-exp: a query far from every data row has a finite result where the density itself underflows.
 *   z (n rows), zq (m rows): WHITENED and centred float64 rows of d values, row strides ldz, ldq >= d.
 *   logw (n) or NULL (all zero).  A -inf entry is a row that is no part of the sample, whatever it holds.
 *   exclude_self: the term j == i is left out (the leave-self-out density at the data rows); needs zq == z, ldq == ldz, m == n.
 *   work: bfhip_kde_work_bytes(n, m, d) bytes of the caller's, 256-byte aligned (0: arguments that bfhip_kde_logsum refuses).
 * Energies are (|zq_i|^2 + |z_j|^2) / 2 - zq_i . z_j with the dot products on the float64 matrix cores.  The data rows are cut into
 * parts by n alone and every sum has an order fixed by (n, d): a query's result depends on that query and the data only -- bit for
 * bit the same alone, in any batch, at any offset -- and few queries still spread over the device.  No atomics; stream-ordered, no
 * host synchronisation.  A NaN in a query row makes that output NaN and no other; a NaN or an infinity in a data row of weight above
 * -inf, or a NaN or +inf in logw, makes every output NaN.  Every weight -inf: every output -inf.
 * BFHIP_ERR_ARG: n, m or d < 1, a stride below d, exclude_self on other queries, a small work buffer.  BFHIP_ERR_UNSUPPORTED:
 * d > BFHIP_MAX_DIM; n or m > 2^31 - 1. */
size_t bfhip_kde_work_bytes(long n, long m, int d);
int bfhip_kde_logsum(bfhip_ctx *ctx, int d, long n, const double *z, long ldz, const double *logw, long m, const double *zq, long ldq,
                     int exclude_self, double *out, void *work, size_t work_bytes);

/* Kernel-weighted means over the same pairs, in one pass: with t_ij = logw[j] - |zq_i - z_j|^2 / 2,
 *     logsum[i] = log sum_j exp(t_ij),   mean[i][c] = sum_j exp(t_ij - logsum[i]) v[j][c],   c < k.
 * With v = z this is the score of the estimate (grad log p = A (mean - zq_i), A the whitening factor) and the mean-shift step; with
 * any per-row quantity it is Nadaraya-Watson kernel regression, and with exclude_self its cross-validated prediction at the rows.
 *   z, logw, zq, exclude_self: as in bfhip_kde_logsum.
 *   v (n rows of k values, row stride ldv >= k), 1 <= k <= BFHIP_MAX_DIM (batch wider v); v == z (with ldv == ldz, k == d) is allowed
 *   and is the common case: nothing more is staged then.
 *   logsum (m) or NULL; mean (m rows of k values, row stride ldo >= k).
 *   work: bfhip_kde_wmean_work_bytes(n, m, d, k) bytes of the caller's, 256-byte aligned (0: arguments that bfhip_kde_wmean refuses).
 * The data rows are cut into parts as in bfhip_kde_logsum; a part leaves (maximum, sum, k numerators) per query, merged in increasing
 * part number; the queries of one launch shrink so that these partials stay below 64 MB, which changes no bit.  Every sum has an
 * order fixed by (n, d, k): a query gives the same bits alone, in any batch, at any offset.  No atomics; stream-ordered.
 * A row of weight -inf is no part of the sample, whatever z and v hold there.  A NaN or +inf weight, or a non-finite z row of weight
 * above -inf, makes every output NaN; a non-finite v[j][c] in such a row makes column c NaN for every query; a NaN in a query row
 * makes that query's outputs NaN.  A query with no term (exclude_self with one weighted row) has logsum -inf and a NaN mean.
 * BFHIP_ERR_ARG: n, m, d or k < 1, a null pointer, ldz or ldq < d, ldv or ldo < k, exclude_self on other queries, a small work
 * buffer.  BFHIP_ERR_UNSUPPORTED: d or k > BFHIP_MAX_DIM; n or m > 2^31 - 1. */
size_t bfhip_kde_wmean_work_bytes(long n, long m, int d, int k);
int bfhip_kde_wmean(bfhip_ctx *ctx, int d, long n, const double *z, long ldz, const double *logw, int k, const double *v, long ldv, long m,
                    const double *zq, long ldq, int exclude_self, double *logsum, double *mean, long ldo, void *work, size_t work_bytes);

/* One pass of expectation-maximisation for a mixture of k Gaussians over n draws: the E step and the sufficient statistics of the M
 * step (nothing in the reference; bayesfast_amd/utils/gmm.py).  With t_ik = logc[k] - |(x_i - mean_k) A_k|^2 / 2:
 *     logpdf[i] = log sum_k exp(t_ik),   resp[i][k] = exp(t_ik - logpdf[i]),
 * a true log-sum-exp with a running maximum: a row so far from every component that every exp(t_ik) underflows still has a finite
 * logpdf and responsibilities that sum to 1.  The energy is formed from the DIFFERENCE x_i - mean_k, subtracted before the product
 * with A_k; the quadratic form is not expanded, so a component far from the origin loses no digits to cancellation.
 *   x (n rows of d values, row stride ldx >= d): a strided view of the chain tensor goes in as it is.
 *   logw (n) or NULL (all zero): log weights, normalised by the caller.
 *   centre (d): the caller's common centre of the moments (the weighted mean of the sample).
 *   mean (k x d); whiten: k matrices A_k (d x d, row-major) with Sigma_k^-1 = A_k A_k^T;
 *   logc[k] = log pi_k + log|det A_k| - d/2 log 2 pi.
 * Outputs, each may be NULL but not all three:
 *   logpdf (n); resp (n rows of k values, row stride ldr >= k);
 *   stats (k (1 + d + d d) + 2): with w_i = exp(logw[i]), N_j = sum_i w_i r_ij at [j], S1_j = sum_i w_i r_ij (x_i - c) at
 *   [k + j d ..], S2_j = sum_i w_i r_ij (x_i - c)(x_i - c)^T at [k (1 + d) + j d d ..] (j the component), then sum_i w_i logpdf[i]
 *   and sum_i w_i.  S2_k is stored full and EXACTLY symmetric: the upper tiles are computed and mirrored.
 *   work: bfhip_gmm_work_bytes(n, d, k) bytes of the caller's, 256-byte aligned (0: arguments that bfhip_gmm_step refuses): 8 n k
 *   bytes (t_ik, then w_i r_ik in its place), 16 bytes per 64 rows, and the partial statistics of at most 128 parts of rows.
 * logpdf and resp do not look at logw; a row with a non-finite value has a NaN logpdf and NaN responsibilities.  In stats a row of
 * weight -inf is no part of the sample, whatever it holds, NaN included; a NaN or +inf weight, or a non-finite row of weight above
 * -inf, makes every entry of stats NaN.  The rows are cut into parts by n alone and every sum of stats has an order fixed by
 * (n, d, k): the waves are folded first, then the parts, in increasing order, without atomics, so stats is bitwise repeatable; a row's
 * logpdf and resp depend on that row and the parameters only -- the same bits alone, in any batch, at any offset.  Stream-ordered,
 * no host synchronisation.
 * BFHIP_ERR_ARG: n, d or k < 1, a null input, ldx < d, ldr < k, all three outputs NULL, a small or misaligned work buffer.
 * BFHIP_ERR_UNSUPPORTED: d > BFHIP_MAX_DIM; k > BFHIP_GMM_MAX_K; n > 2^31 - 1. */
#define BFHIP_GMM_MAX_K 32
size_t bfhip_gmm_work_bytes(long n, int d, int k);
int bfhip_gmm_step(bfhip_ctx *ctx, int d, int k, long n, const double *x, long ldx, const double *logw, const double *centre,
                   const double *mean, const double *whiten, const double *logc, double *stats, double *logpdf, double *resp, long ldr,
                   void *work, size_t work_bytes);

/* The normal quantile function of n probabilities, out[i] = ndtri(p[i]) (scipy.special.ndtri, which scipy.stats.norm.ppf evaluates:
 * utils/sobol.py:57 on the Sobol points of multivariate_normal, transforms/sit.py:225 on the KDE cdfs): Cephes' algorithm; -inf / +inf
 * at 0 / 1, NaN outside [0, 1].  p and out may be the same array. */
int bfhip_ndtri(bfhip_ctx *ctx, long n, const double *p, double *out);

/* The Gaussianizing splines of one SIT iteration, all d coordinates in one launch (SIT._gaussianize_1d, transforms/sit.py:223-227:
 * cubic_spline(x, lambda xx: norm.ppf(kde.cdf(xx)), **cubic_options), utils/cubic.py:19-260).  sorted (d,n): every coordinate's
 * samples in ascending order (the percentiles); data (d,n), w (n) normalised, h (d): the KDE as in bfhip_kde_cdf.  grid (n_grid):
 * np.linspace(0, 100, bins + 1)[edge_bins:-edge_bins]; inner (n_inner): np.linspace(0, 100, edge_points + 2)[1:-1]; edge_bins,
 * max_width, split, max_add: cubic_spline's options.  Output per coordinate j: out_n[2 j] knots (0 when the coordinate was given up),
 * out_n[2 j + 1] flags (1 too few distinct knots / nothing beyond the edge knots, 2 singular slope system, 4 'the knots are too
 * unevenly spaced' (the reference raises), 8 more than 512 knots, 16 'Not all the intervals are monotone' (the reference warns));
 * knots out_x[j stride ..], values out_y[j stride ..], coefficient rows out_c[j 4 (stride + 1) ..] (m + 1 rows of 4, as
 * bfhip_spline_apply takes them).  stride >= 512, n_grid <= 512, n_inner <= 128. */
int bfhip_spline_build(bfhip_ctx *ctx, int d, long n, const double *sorted, const double *data, const double *w, const double *h,
                       int n_grid, const double *grid, int edge_bins, int n_inner, const double *inner, double max_width, int split,
                       int max_add, int stride, double *out_x, double *out_y, double *out_c, int *out_n);

/* The per-dimension piecewise cubics of SIT for n points x (n,d) -> out (n,d): mode 0 evaluate, 1 derivative, 2 solve
 * (utils/_cubic.pyx:188-336, called per dimension by SIT.forward_transform / backward_transform, transforms/sit.py:372-451).
 * Dimension j owns knots[knot_off[j] .. knot_off[j+1]), values there, and m_j + 1 coefficient rows of 4 at
 * coef[(knot_off[j] + j) * 4] (cubic_spline._x, ._y, ._c of utils/cubic.py).  knot_off (d+1,) int32. */
int bfhip_spline_apply(bfhip_ctx *ctx, int mode, long n, int d, const double *x, const int *knot_off, const double *knots,
                       const double *values, const double *coef, double *out);

/* Score function of the bridge estimator (evidence/bridge.py:44-49): out2[0] = logsumexp_i(logr + a_i - logaddexp(logr + a_i, 0)),
 * out2[1] = logsumexp_j(-logr + b_j - logaddexp(-logr + b_j, 0)); score = out2[0] - out2[1]. */
int bfhip_bridge_sums(bfhip_ctx *ctx, long n_a, const double *a, long n_b, const double *b, double logr, double *out2);

/* Per-sample terms of its error estimate (evidence/bridge.py:52-57): f1 (n_q), f2 (n_p). */
int bfhip_bridge_terms(bfhip_ctx *ctx, long n_p, const double *logp_p, const double *logq_p, long n_q, const double *logp_q,
                       const double *logq_q, double logr, double *f1, double *f2);

/* Importance sampling (evidence/importance.py:26-28, x = logp_q, y = logq_q) and the harmonic mean (evidence/harmonic.py:27-31,
 * x = logq_p, y = logp_p, log r = -L): with t_i = x_i - y_i (i < n), out3[0] = L = log(mean_i exp(t_i)); out3[1] = mean_i f_i,
 * out3[2] = population variance of f_i (numpy's ddof = 0), where f_i = exp(t_i - L); terms (may be NULL) receives f_i.
 * -inf in t is a zero weight, NaN propagates; when every t_i is -inf, L = -inf and the moments are NaN.  Fixed-order reductions
 * (bitwise repeatable), stream-ordered, no host synchronisation. */
int bfhip_logmeanexp_stats(bfhip_ctx *ctx, long n, const double *x, const double *y, double *out3, double *terms);

/* The glue of one FastICA iteration (scikit-learn's _ica_par, logcosh contrast, as SIT calls it: transforms/sit.py:235-244) around
 * the caller's two products Y = X1 W^T and P[b] = G_b^T X1_b (row batches b) and bfhip_polar_ns:
 *   bfhip_ica_tanh      y (n_pad,d) <- tanh(y) in place; partial (ceil(n_pad / 32), d) <- column sums of 1 - tanh(y)^2 over the
 *                       rows < n of every block of 32 rows (rows n .. n_pad: zero padding, not counted)
 *   bfhip_ica_assemble  a (d,d) <- (sum_b p[b]) / n - gmean[:, None] w,  gmean = column sums of partial / n;  p (nb,d,d);
 *                       *meas_k <- 0 (the slot bfhip_ica_post reduces into; may be NULL)
 *   bfhip_ica_post      meas[k] <- max(meas[k], max_i | |sum_j w1[i][j] w[i][j]| - 1 |), meas[n_meas + k] <- resid[0];
 *                       wbuf[k] <- w1; w <- w1 */
int bfhip_ica_tanh(bfhip_ctx *ctx, long n, long n_pad, int d, double *y, double *partial);
int bfhip_ica_assemble(bfhip_ctx *ctx, int d, int nb, const double *p, long n, long n_pad, const double *partial, const double *w,
                       double *a, double *meas_k);
int bfhip_ica_post(bfhip_ctx *ctx, int d, const double *w1, double *w, const double *resid, int k, int n_meas, double *wbuf,
                   double *meas);

/* FastICA's symmetric decorrelation W <- (W W^T)^{-1/2} W (sklearn.decomposition FastICA, as SIT calls it: transforms/sit.py:235-244;
 * scikit-learn takes an eigen-decomposition of W W^T on the host in every fixed-point iteration): the orthogonal polar factor of
 * a (d,d), by AT MOST n_iter Newton-Schulz steps on the FP64 matrix cores (the iteration stops once max |x x^T - I| < 1e-13), into
 * x (d,d).  work: 2 d^2 + n_iter + 10 doubles (the iterates' second buffer, the grid barrier's counter, a residual per step: all
 * in the caller's memory, so that a HIP graph holding the launch stays valid); resid (1,) receives max |x x^T - I| (device memory:
 * nothing synchronises; a caller checks it when it next looks at the device).  d <= 1024. */
int bfhip_polar_ns(bfhip_ctx *ctx, int d, const double *a, double *x, int n_iter, double *work, double *resid);

/* The integrated autocorrelation time of many chains (utils/acor.py:79-145, integrated_time: emcee's estimator with Sokal's
 * automatic window; the reference's PostStep calls it, core/recipe.py:1304): the two reductions over walkers and time behind it.
 * x: n_w walkers of (n_t, n_d) float64 each, walker w at x + w ldw (ldw >= n_t n_d, so that samples[:, since:] goes in as it is),
 * every walker's block row-major and contiguous.  y_wk(s) = x_wk(s) - mean_wk, a_wk(t) = sum_{s < n_t - t} y_wk(s) y_wk(s + t).
 *   bfhip_acor_moments   mean (n_w, n_d) <- mean_wk; inv (n_w, n_d) <- 1 / a_wk(0), both by two passes over time (a constant series
 *                        has inv = inf, and its lag sums are NaN, as the host port's 0 / 0)
 *   bfhip_acor_lag_sums  out (n_lag, n_d) <- sum_w a_wk(t0 + i) inv_wk for i < n_lag (exactly +0 for lags >= n_t, whatever the
 *                        series holds); mean and inv from bfhip_acor_moments.  work: min(n_w, 256) n_lag n_d doubles
 *                        (per-walker-group partial sums).  A series with a NaN or an infinite sample has NaN moments, and its
 *                        column is NaN at every lag < n_t.  With a finite mean supplied by the caller instead, such a sample
 *                        makes NaN every lag whose sum contains it, and may make NaN any other lag < n_t of its column (the
 *                        zero padding past the series' end multiplies it): which of those is not part of the contract, and
 *                        the independence of the block below does not cover them.  Other columns are never touched by it.
 * The window search (rho_k = out / n_w, tau_k(t) = 2 sum rho_k - 1, the first t >= c tau_k(t)) is the caller's: it asks for lag
 * blocks until every window has closed.  n_d >= 1 of any size (BFHIP_MAX_DIM does not apply); NaN propagates.  Every sum has a
 * fixed order set by (n_w, n_t, n_d) alone: bitwise repeatable, and a lag's sum does not depend on the block that computes it.
 * Work: n_w n_t n_d reads twice (moments); n_w n_d n_lag (n_t - t0) FMAs and n_w n_t n_d reads per 64 lags (lag sums).
 * Stream-ordered, no host synchronisation. */
int bfhip_acor_moments(bfhip_ctx *ctx, int n_w, long n_t, int n_d, long ldw, const double *x, double *mean, double *inv);
int bfhip_acor_lag_sums(bfhip_ctx *ctx, int n_w, long n_t, int n_d, long ldw, const double *x, const double *mean, const double *inv,
                        long t0, int n_lag, double *work, double *out);

/* Did the sampler itself work (bayesfast_amd/utils/health.py, sampler_health: the divergent transitions, the transitions that hit
 * the tree-depth limit and Betancourt's E-BFMI that Stan, PyMC and ArviZ warn about): the per-chain figures, in one launch, from
 * the statistics table as bfhip_sampler_run left it.
 * stats: the FIRST SELECTED ROW of chain 0; chain c's n_rows rows of BFHIP_STAT_STRIDE float64 start at stats + c ldc and are
 * contiguous (ldc >= n_rows BFHIP_STAT_STRIDE doubles, free for one chain), so that a [:, since:] view of a longer table goes in as
 * it is.  sampler: 0 = NUTS (the BFHIP_NS_* columns), 1 = HMC (BFHIP_HS_*).  1 <= max_treedepth <= BFHIP_MAX_TREEDEPTH.
 *   out_i (n_chain, BFHIP_HEALTH_I_N) int64, exact:
 *     N_DIVERGENT       rows with diverging != 0
 *     N_MAX_TREEDEPTH   NUTS: rows with tree_depth >= max_treedepth; HMC: 0
 *     N_LEAPFROG        sum of tree_size (HMC: of n_int_step); an entry that is no positive number below 2^52 counts as 0
 *     MAX_TREE_SIZE     the largest of them
 *     N_ACCEPTED        HMC: rows with accepted != 0; NUTS: 0
 *     N_NONFINITE       rows whose logp or energy is not finite
 *     N_MOVED           rows i >= 1 whose logp differs from that of row i - 1 (0: the chain never moved; an exact test, where
 *                       the centred sum of squares of n copies of a constant depends on how their sum rounds)
 *     DEPTH_HIST + b    NUTS: rows with tree_depth in [b, b + 1), b = 0 .. BFHIP_MAX_TREEDEPTH; a depth outside [0,
 *                       BFHIP_MAX_TREEDEPTH] (or NaN) is counted in the last bin; HMC: 0
 *   out_f (n_chain, BFHIP_HEALTH_F_N) float64:
 *     MEAN_ACCEPT       mean of mean_tree_accept (HMC: of accept_stat)
 *     LOGP_MEAN, LOGP_VAR, ENERGY_MEAN, ENERGY_VAR   the variances unbiased (n_rows - 1), each a second pass about its mean
 *     BFMI              sum_{i >= 1} (E_i - E_{i-1})^2 / sum_i (E_i - mean E)^2 (a constant energy: NaN, the 0 / 0 it stands for, whatever
 *                       the rounding of the mean leaves in the denominator)
 *     STEP_SIZE         step_size of the last selected row
 *   A chain with N_NONFINITE > 0 has NaN in its five moments and BFMI (MEAN_ACCEPT and STEP_SIZE are what the table holds); no
 *   other chain is touched by it.
 * One workgroup per chain; every sum has an order set by n_rows alone, so a chain's outputs are the same bits alone or in any
 * launch, at any chain index.  n_chain >= 1, 2 <= n_rows <= 2^38.  Work: the selected rows are read twice (the second time from
 * cache).  Stream-ordered, no host synchronisation, no atomics. */
enum {
    BFHIP_HEALTH_I_N_DIVERGENT = 0, BFHIP_HEALTH_I_N_MAX_TREEDEPTH, BFHIP_HEALTH_I_N_LEAPFROG, BFHIP_HEALTH_I_MAX_TREE_SIZE,
    BFHIP_HEALTH_I_N_ACCEPTED, BFHIP_HEALTH_I_N_NONFINITE, BFHIP_HEALTH_I_N_MOVED, BFHIP_HEALTH_I_DEPTH_HIST,
    BFHIP_HEALTH_I_N = BFHIP_HEALTH_I_DEPTH_HIST + BFHIP_MAX_TREEDEPTH + 1
};
enum {
    BFHIP_HEALTH_F_MEAN_ACCEPT = 0, BFHIP_HEALTH_F_LOGP_MEAN, BFHIP_HEALTH_F_LOGP_VAR, BFHIP_HEALTH_F_ENERGY_MEAN,
    BFHIP_HEALTH_F_ENERGY_VAR, BFHIP_HEALTH_F_BFMI, BFHIP_HEALTH_F_STEP_SIZE, BFHIP_HEALTH_F_N
};
int bfhip_health_chains(bfhip_ctx *ctx, int n_chain, long n_rows, long ldc, const double *stats, int sampler, int max_treedepth,
                        long long *out_i, double *out_f);

/* Convergence diagnostics of many chains (rank-normalised split-R-hat, bulk / tail / mean effective sample size and the table of
 * mean, sd and quantiles: Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; bayesfast_amd/utils/diagnostics.py holds the
 * estimators and the walk over Geyer's sequence).  The data-sized passes, on a batch of at most BFHIP_DIAG_BATCH parameters:
 *   bfhip_diag_columns  columns k0 .. k0 + nb - 1 of the time-major sample tensor -> out (2 n_chain, h, BFHIP_DIAG_BATCH), the
 *                       split layout: chain c's rows since .. since + h - 1 are split chain 2 c, the next h rows split chain
 *                       2 c + 1.  Element (c, row r, column k) is x[c ldw + r ldr + k] (ldr >= the row length, ldw free: a
 *                       [:, since:] view goes in without a copy); x is float64, or float32 (is_f32) read as float64.
 *                       mode BFHIP_DIAG_PLAIN: x; BFHIP_DIAG_FOLD: |x - c[b]|; BFHIP_DIAG_BELOW: 1 if x <= c[b], else 0 (c (nb,)
 *                       device constants, one per column; not read in the plain mode).  Columns nb .. BFHIP_DIAG_BATCH - 1 of out
 *                       are written as 0, so that every batch has one shape and the reductions over it one order.
 *   bfhip_diag_extent   lo, hi (n_series, BFHIP_DIAG_BATCH) <- the smallest and the largest value of every split chain's column of a
 *                       (n_series, h, BFHIP_DIAG_BATCH) series buffer (NaN draws are passed over; a column of NaN alone gives
 *                       lo = inf, hi = -inf).  A parameter is constant exactly when the smallest lo equals the largest hi: an
 *                       exact comparison, where the centred sum of squares of n copies of a constant depends on how their sum rounds.
 *   bfhip_diag_sort     stable ascending sort of column b of a (n, BFHIP_DIAG_BATCH) series buffer: keys_sorted (n,) uint64 (the
 *                       order-preserving keys of bfhip_sort_keys: every NaN last, -0 == +0), order (n,) uint32 the permutation.
 *                       n <= 2^31 - 1.  The quantiles are read off keys_sorted.
 *   bfhip_diag_rank     z[order[p] BFHIP_DIAG_BATCH + b] = ndtri((r_p - 3/8) / (n + 1/4)) for every sorted position p, r_p the
 *                       1-based rank, tied values sharing the mean of their ranks (the tie run by lower / upper bound in
 *                       keys_sorted).  z may be the buffer the column was sorted from.
 * The chain moments and autocovariance sums of a series buffer are bfhip_acor_moments and bfhip_acor_lag_sums with n_w = 2 n_chain,
 * n_t = h, n_d = BFHIP_DIAG_BATCH, ldw = h BFHIP_DIAG_BATCH and inv filled with 1.  Stream-ordered, no host synchronisation; every
 * result is bitwise repeatable and does not depend on the batch or the column a parameter lands in. */
#define BFHIP_DIAG_BATCH 16
#define BFHIP_DIAG_PLAIN 0
#define BFHIP_DIAG_FOLD 1
#define BFHIP_DIAG_BELOW 2
int bfhip_diag_columns(bfhip_ctx *ctx, int n_chain, long h, long ldw, long ldr, const void *x, int is_f32, long since, int k0, int nb,
                       int mode, const double *c, double *out);
int bfhip_diag_extent(bfhip_ctx *ctx, int n_series, long h, const double *series, double *lo, double *hi);
int bfhip_diag_sort(bfhip_ctx *ctx, long n, const double *series, int b, uint64_t *keys_sorted, uint32_t *order);
int bfhip_diag_rank(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, const uint32_t *order, int b, double *z);

/* Pareto-smoothed importance sampling (Vehtari, Simpson, Gelman, Yao, Gabry 2024; bayesfast_amd/utils/psis.py has the definitions) of
 * n log ratios lw = logp - logq (logq NULL: logp holds the ratios), all (n,) float64 on the device, n <= 2^31 - 1.  One call, one fixed
 * launch sequence (the tail size M = min(n / 5, ceil(3 sqrt n)) and the m = 30 + floor(sqrt M) candidate thetas follow from n):
 * the ratios, their maximum and a flag for a NaN or +inf; the shift by the maximum; the stable sort of bfhip_sort_keys; the
 * generalised-Pareto fit of Zhang & Stephens (2009) to the M largest exceedances exp(lw) - exp(cut) over the value at sorted position
 * n - M - 1 -- a workgroup per theta_j reduces log1p(-theta_j x_i), one workgroup forms the profile likelihoods, their weights, theta,
 * k, sigma = -k / theta and khat = (k M + 5) / (M + 10); the scatter of log(exp(cut) + sigma expm1(-khat log1p(-p_i)) / khat),
 * p_i = (i - 1/2) / M, capped at 0, through the sort's permutation; a two-level logsumexp and sum of squares; the normalisation.
 *   lw_out (n,)  the smoothed log weights, logsumexp 0, in the input's order (also the call's working copy of the ratios)
 *   out8 (8,)    khat, sigma, M, cut, log mean weight (maximum + logsumexp - log n of the smoothed, shifted values: the estimate of
 *                log Z_p / Z_q), the Kish effective sample size 1 / sum w^2, the maximum that was subtracted, flags
 *                (1: a NaN or +inf ratio, or no ratio above -inf -- every output is NaN; 2: no smoothing -- M < 5 or a tail without
 *                spread -- khat = inf, sigma = NaN)
 *   work         BFHIP_PSIS_WORK_BYTES(n) bytes of the caller's, 8-byte aligned: sorted keys, permutation, partial results
 * -inf ratios are zero weights, sort first and count in n.  Every reduction has a fixed order (a thread adds in index order, a
 * workgroup by a halving tree, one workgroup the at most 1024 partial results): bitwise repeatable.  Stream-ordered; the sort
 * keeps its temporary storage in the context's workspace, which synchronises only when it has to grow. */
#define BFHIP_PSIS_WORK_BYTES(n) (16 * (size_t)(n) + 32768)
int bfhip_psis(bfhip_ctx *ctx, long n, const double *logp, const double *logq, double *lw_out, double *out8, void *work,
               size_t work_bytes);

/* The weighted table of mean, sd and quantiles (bayesfast_amd/utils/psis.py: weighted_summary), on a batch of at most
 * BFHIP_DIAG_BATCH parameters and weights w (n,) >= 0 that sum to 1:
 *   bfhip_wstat_columns     columns k0 .. k0 + nb - 1 of the time-major sample tensor -> out (n_chain n_draw, BFHIP_DIAG_BATCH), row
 *                           c n_draw + i <- x[c ldw + (since + i) ldr + k], the addressing of bfhip_diag_columns (float64, or float32
 *                           read as float64; a [:, since:] view goes in without a copy) but without the split: every draw is kept.
 *                           Columns nb .. BFHIP_DIAG_BATCH - 1 are written as 0.  With w (n,) given (it may be NULL) the rows of zero
 *                           weight are written as NaN: they are not part of the weighted sample whatever they hold, and sort last.
 *   bfhip_wstat_moments     series NULL: wsum (4,) <- sum w, sum w^2, the number of non-zero weights, 1 if a weight is negative or not
 *                           finite -- computed once per weight vector.  series (n, BFHIP_DIAG_BATCH): out (5, BFHIP_DIAG_BATCH) <-
 *                           per column sum w x, then on a second pass over the data sum w (x - mean)^2 and sum w^2 (x - mean)^2, and
 *                           the smallest and the largest value, all over the rows of non-zero weight (a NaN among them shows in the
 *                           sums, not in the extremes).  work: BFHIP_WSTAT_WORK doubles.
 *   bfhip_wstat_cumweights  cum[p] = sum_{p' <= p} w[order[p']] for the permutation order (n,) of bfhip_diag_sort.  Three launches:
 *                           the sums of tiles of 2048 sorted positions, their scan by ONE workgroup, the final pass; no workgroup
 *                           waits on another, any n <= 2^31 - 1.  Exact for whole-number weights.  work: ceil(n / 2048) doubles.
 *   bfhip_wstat_quantiles   out[i BFHIP_DIAG_BATCH + b] <- the weighted quantile at probs[i] (nq device doubles in [0, 1]) over the
 *                           first wsum[2] sorted positions: with mid_k = cum[k] - w_(k) / 2 and pos_k = (mid_k - mid_first) /
 *                           (mid_last - mid_first), k the last position with pos_k <= q by bisection, the value interpolated linearly
 *                           between positions k and k + 1 (the last value for the last k); values decoded from keys_sorted.
 * Stream-ordered, no host synchronisation; fixed-order reductions in which a column never meets its neighbours: bitwise
 * repeatable, whichever batch or column a parameter lands in. */
#define BFHIP_WSTAT_WORK 65536
int bfhip_wstat_columns(bfhip_ctx *ctx, int n_chain, long n_draw, long ldw, long ldr, const void *x, int is_f32, long since, int k0,
                        int nb, const double *w, double *out);
int bfhip_wstat_moments(bfhip_ctx *ctx, long n, const double *series, const double *w, double *wsum, double *out, double *work);
int bfhip_wstat_cumweights(bfhip_ctx *ctx, long n, const uint32_t *order, const double *w, double *cum, double *work);
int bfhip_wstat_quantiles(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, const uint32_t *order, const double *w, const double *cum,
                          const double *wsum, int nq, const double *probs, int b, double *out);

/* Pointwise leave-one-out cross-validation by Pareto-smoothed importance sampling, and WAIC (Vehtari, Gelman, Gabry 2017;
 * bayesfast_amd/utils/data_loo.py has the definitions), of a batch of nb <= BFHIP_DIAG_BATCH columns of pointwise log likelihoods in a
 * series buffer: element (row s, column b) at series[s ld + b], ld >= nb, n rows, n <= 2^31 - 1 (BFHIP_ERR_UNSUPPORTED beyond).
 *   mode  BFHIP_PLOO_ELL: the buffer holds ell_s.  BFHIP_PLOO_Z: it holds z_s and ell_s = c[b] - z_s^2 / 2, c (BFHIP_DIAG_BATCH,) on the device.
 *   lb    (n,) device base log weights, logsumexp 0, or NULL: -log n each.  A row with lb = -inf is not part of the sample, whatever it
 *         holds; it counts in n.  The importance ratio that removes the point is r_s = lb_s - ell_s (NULL: -ell_s).
 *   out   (BFHIP_PLOO_NOUT, BFHIP_DIAG_BATCH) doubles, rows BFHIP_PLOO_LPD ... below; the three stages fill it between them, in this order.
 *   work  bfhip_ploo_work_bytes(n) bytes of the caller's, 256-byte aligned, the same buffer for the three stages of a batch.
 * bfhip_ploo_moments: max r, lpd = logsumexp(lb + ell), sum w ell, sum w (ell - sum w ell)^2 on a second pass, sum w^2, max lb and the
 *   flags 1 (a non-finite ell in a row of non-zero weight) and 4 (no row of non-zero weight).
 * bfhip_ploo_tail: with M = min(n / 5, ceil(3 sqrt n)), the M + 1 largest ratios r_s - max r of every column in the order of a stable
 *   ascending sort of the column (among equal keys the lower row first): tail_keys (BFHIP_DIAG_BATCH, M + 1) uint64 order-preserving
 *   keys, ascending, and tail_idx (BFHIP_DIAG_BATCH, M + 1) uint32 rows; position 0 is the cut of bfhip_psis, sorted position n - M - 1.
 *   A most-significant-digit radix select over the keys (eight histogram passes with integer counters), a compaction of the rows above
 *   the cut pair, and two segmented sorts of those M pairs; no column is sorted.  Reads out's BFHIP_PLOO_MAXR row.
 * bfhip_ploo_finish: per column the generalised-Pareto fit of bfhip_psis on the tail keys (same kernels, same arithmetic), the smoothed
 *   tail values, and the sums behind elpd_loo = logsumexp(v + ell), ess_loo = 1 / sum exp(2 v) and pit = sum exp(v) Phi(z) (Z mode; NaN
 *   in ELL mode) for the smoothed, normalised log weights v: rows not above the cut pair with their own ratio in one pass over the
 *   batch, the M tail rows with their smoothed value, fetched by index.  Flag 2: nothing smoothed (M < 5 or a tail without spread;
 *   khat = inf).  With flag 1 or 4 every figure of the column but M is NaN.
 * Every floating-point reduction has an order fixed by n alone and a column never meets its neighbours: bitwise repeatable, whichever
 * slot or batch a column lands in.  Stream-ordered, no host synchronisation (the sorts keep their temporary storage in the context's
 * workspace, which synchronises only when it has to grow). */
#define BFHIP_PLOO_ELL 0
#define BFHIP_PLOO_Z 1
#define BFHIP_PLOO_NOUT 16
#define BFHIP_PLOO_LPD 0      /* logsumexp(lb + ell) */
#define BFHIP_PLOO_SWE 1      /* sum w ell, w = exp(lb) */
#define BFHIP_PLOO_WAIC 2     /* sum w (ell - sum w ell)^2 */
#define BFHIP_PLOO_ELPD 3     /* elpd_loo */
#define BFHIP_PLOO_KHAT 4
#define BFHIP_PLOO_SIGMA 5
#define BFHIP_PLOO_M 6
#define BFHIP_PLOO_CUT 7      /* the cut, r - max r at sorted position n - M - 1 */
#define BFHIP_PLOO_ESS 8      /* 1 / sum exp(2 v) */
#define BFHIP_PLOO_PIT 9
#define BFHIP_PLOO_MAXR 10    /* max r */
#define BFHIP_PLOO_FLAGS 11
#define BFHIP_PLOO_SW2 12     /* sum w^2 */
#define BFHIP_PLOO_MAXB 13    /* max lb; rows 14 and 15 are the stages' own */
size_t bfhip_ploo_work_bytes(long n);
int bfhip_ploo_moments(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                       double *out, void *work, size_t work_bytes);
int bfhip_ploo_tail(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                    const double *out, uint64_t *tail_keys, uint32_t *tail_idx, void *work, size_t work_bytes);
int bfhip_ploo_finish(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                      const uint64_t *tail_keys, const uint32_t *tail_idx, double *out, void *work, size_t work_bytes);

/* The posterior reweighted to a batch of nb <= BFHIP_DIAG_BATCH columns of log ratios l (bayesfast_amd/utils/reweight.py has the
 * definitions): a third stage in place of bfhip_ploo_finish.  The series buffer holds -l in mode BFHIP_PLOO_ELL, so that the ratio of
 * bfhip_ploo_moments and bfhip_ploo_tail, lb - ell, is r = lb + l; out, tail_keys and tail_idx are what those two stages left (out is
 * only read), work their work buffer.  The fit and the smoothed tail are launched exactly as bfhip_ploo_finish launches them: khat,
 * sigma, the cut and the flags are its figures, bit for bit.
 *   draws    read in place as bfhip_wstat_columns reads them: series row s is draw (s / n_draw, s % n_draw), parameter j at
 *            x[(s / n_draw) ldw + (since + s % n_draw) ldr + j], float64 or float32 (is_f32); n_chain n_draw == n, ldr >= d, 1 <= d <= BFHIP_MAX_DIM
 *   centre   (d,) device doubles c: the sums are taken about it
 *   rw_out   (BFHIP_RW_NOUT(d), BFHIP_DIAG_BATCH) doubles: rows BFHIP_RW_LER ... below, then from row BFHIP_RW_SUMS on the 1 + 2 d sums
 *            sum e, sum e (x_j - c_j) (j < d), sum e (x_j - c_j)^2 (j < d), and the same 1 + 2 d with e^2, for e = exp(v) of the smoothed
 *            shifted ratios v (the caller normalises: w = e / sum e).  Columns nb .. are not written.
 *   rw_work  bfhip_rw_work_bytes(n, d) bytes of the caller's, 256-byte aligned
 * Rows not above the cut pair go through one pass on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, four rows a step: e of the sixteen
 * columns against [1, x - c, (x - c)^2] in tiles of 16), the M tail rows are fetched by index with their smoothed values.  A row with
 * lb = -inf is in no sum of rw_out's rows from BFHIP_RW_SUMS on (where the tail holds such rows they stay in the sum e and sum e^2 behind
 * BFHIP_RW_LER and BFHIP_RW_ESS, as in bfhip_ploo_finish) and is not read as a number; a non-finite
 * draw in any other row makes that parameter's sums non-finite in every column.  With flag 1 or 4 every figure of the column but M and the
 * flags is NaN.  Every reduction has an order fixed by n and d alone, no atomics, and a column never meets its neighbours: bitwise
 * repeatable, whichever slot or batch a column lands in.  Stream-ordered, no host synchronisation. */
#define BFHIP_RW_LER 0        /* max r + log sum e over every row: the log of the ratio of the evidences */
#define BFHIP_RW_KHAT 1
#define BFHIP_RW_SIGMA 2
#define BFHIP_RW_M 3
#define BFHIP_RW_ESS 4        /* (sum e)^2 / sum e^2 over every row */
#define BFHIP_RW_FLAGS 5      /* as BFHIP_PLOO_FLAGS */
#define BFHIP_RW_CUT 6
#define BFHIP_RW_SUMS 8
#define BFHIP_RW_NOUT(d) (BFHIP_RW_SUMS + 2 * (1 + 2 * (d)))
size_t bfhip_rw_work_bytes(long n, int d);
int bfhip_rw_finish(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                    const uint64_t *tail_keys, const uint32_t *tail_idx, const double *out, void *work, size_t work_bytes, int n_chain,
                    long n_draw, long ldw, long ldr, const void *x, int is_f32, long since, int d, const double *centre, double *rw_out,
                    void *rw_work, size_t rw_work_bytes);

/* Power-scaling sensitivity (bayesfast_amd/utils/power_scale.py has the definitions): the smoothed weights themselves, and the
 * distance between two weighted ECDFs of one parameter for a batch of weight columns.
 * bfhip_rw_weights: a fourth stage after bfhip_ploo_moments and bfhip_ploo_tail, before or after bfhip_rw_finish, with their arguments
 *   (out, tail_keys and tail_idx are only read; work is their work buffer).  u (n, ld_u), ld_u >= nb, a buffer of its own that
 *   overlaps none of the others: u[s ld_u + b] <- e_s / sum over the rows of the sample of e, e = exp(smoothed shifted r) -- rows not
 *   above the cut pair with their own ratio, the M tail rows scattered by index with the smoothed values of the very launches of
 *   bfhip_rw_finish -- and 0 in a row with lb = -inf.  In a column with flag 1 or 4 the rows of the sample are NaN.  Columns nb .. of u
 *   are not written.  wout (BFHIP_RWW_NOUT, BFHIP_DIAG_BATCH): the sum, khat and the flags of bfhip_rw_finish, bit for bit.  The sum is
 *   taken in an order fixed by n alone: bitwise repeatable in any slot of any batch.
 * bfhip_pscale_cjs: one parameter, given by keys_sorted and order (n,) of bfhip_diag_sort on a column of bfhip_wstat_columns under the
 *   base weights w (n,), and wsum of bfhip_wstat_moments (wsum[2] = n_pos, the rows of the sample: the first n_pos sorted positions),
 *   against nb <= BFHIP_DIAG_BATCH columns of weights u (n, ld_u), ld_u >= nb.  With P and Q the running sums of w and u over the sorted
 *   positions (Q - P is the running sum of u - w) and h_p = x_(p+1) - x_(p), p <= n_pos - 2:
 *     out (BFHIP_CJS_NOUT, BFHIP_DIAG_BATCH) rows  BFHIP_CJS_J      sum h [P log2(P / M) + Q log2(Q / M)], M = (P + Q) / 2, as
 *                                                                   M [(1 - t) log1p(-t) + (1 + t) log1p(t)] / ln 2, t = (Q - P) / (P + Q)
 *                                                                   (its even series below |t| = 1/8)
 *                                                  BFHIP_CJS_BOUND  sum h (P + Q)
 *                                                  BFHIP_CJS_CJS    sqrt(J / bound)
 *                                                  BFHIP_CJS_KS     max over h_p > 0 of |P - Q|
 *                                                  BFHIP_CJS_FLAGS  1 a non-finite draw among the rows of the sample, 2 bound == 0
 *                                                                   (either: cjs and ks are NaN)
 *   Columns nb .. of out are not written.  Four launches: the 17 sums (w and the 16 columns of u - w) of tiles of BFHIP_PSCALE_TILE
 *   sorted positions, sixteen lanes to a row of u; their scan by ONE workgroup; the pass that forms every position's terms; the tiles'
 *   partial results reduced by ONE workgroup.  No workgroup waits on another, no atomics, every order fixed by n alone, and a column
 *   never meets its neighbours: bitwise repeatable in any slot.  work: BFHIP_PSCALE_WORK(n) doubles.
 * Stream-ordered, no host synchronisation. */
#define BFHIP_RWW_NOUT 4
#define BFHIP_RWW_SUM 0       /* sum of e over the rows of the sample */
#define BFHIP_RWW_KHAT 1
#define BFHIP_RWW_FLAGS 2     /* as BFHIP_RW_FLAGS; row 3 is spare */
#define BFHIP_CJS_NOUT 5
#define BFHIP_CJS_J 0
#define BFHIP_CJS_BOUND 1
#define BFHIP_CJS_CJS 2
#define BFHIP_CJS_KS 3
#define BFHIP_CJS_FLAGS 4
#define BFHIP_PSCALE_TILE 2048
#define BFHIP_PSCALE_TILE_WORK 352   /* doubles per tile: 17 tile sums, 16 x 17 slice sums, 3 x 16 partial results, padding */
#define BFHIP_PSCALE_WORK(n) ((((size_t)(n) + BFHIP_PSCALE_TILE - 1) / BFHIP_PSCALE_TILE) * BFHIP_PSCALE_TILE_WORK)
int bfhip_rw_weights(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                     const uint64_t *tail_keys, const uint32_t *tail_idx, const double *out, void *work, size_t work_bytes, double *u,
                     long ld_u, double *wout);
int bfhip_pscale_cjs(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, const uint32_t *order, const double *wsum, const double *w,
                     const double *u, long ld_u, int nb, double *out, double *work);

/* Leave-group-out cross-validation of a batch of nb <= BFHIP_DIAG_BATCH groups of data points (bayesfast_amd/utils/data_lgo.py has the
 * definitions).  A group's column of the (n, BFHIP_DIAG_BATCH) series buffer holds ell_s = c - q_s / 2, q_s the conditional chi-square
 * of the group's dof points given the rest at draw s; bfhip_ploo_moments and bfhip_ploo_tail run on it in mode BFHIP_PLOO_ELL.
 * bfhip_igamc: out[i] = Q(a[i], x[i]), the regularised upper incomplete gamma function (the chi-square survival function
 *   Q(dof / 2, q / 2)), a, x, out (n,) device doubles: a series below max(a, 1), a continued fraction above, at most 5000 terms; Q(a, 0)
 *   = 1, Q(a, inf) = 0, NaN for a NaN argument, a <= 0 or x < 0.
 * bfhip_lgo_accum: folds the (n, nb) buffer z (element (s, j) at z[s ldz + j], ldz >= nb) of whitened residuals into acc (element (s,
 *   slot) at acc[s lda + slot], lda >= BFHIP_DIAG_BATCH): column j goes to slot slot[j] (HOST array of nb ints; -1: to none), and the
 *   running value of (row, slot) is updated once per column in column order as acc = acc - 0.5 * (z * z), never contracted.  A slot
 *   whose bit of start is set starts in this call from c[slot] (HOST array of BFHIP_DIAG_BATCH doubles; may be NULL when start is 0),
 *   whatever acc holds; the other slots go on from what acc holds.  Slots that neither start nor take a column are not touched.  The
 *   bits of a column therefore depend on the order of its z columns alone, not on how they were split over calls, slots or batches.
 *   Rows are read and written two doubles at a time where both strides are even and both bases 16-byte aligned.  No atomics.
 * bfhip_lgo_finish: the third stage in place of bfhip_ploo_finish.  c, dof: HOST arrays of nb doubles, dof > 0.  The fit and the
 *   smoothed tail are launched exactly as bfhip_ploo_finish launches them and out gets bfhip_ploo_finish's rows (BFHIP_PLOO_PIT is
 *   NaN); lgo_out (BFHIP_LGO_NOUT, BFHIP_DIAG_BATCH) doubles gets, with q = max(2 (c - ell), 0) and Q = Q(dof / 2, q / 2), the rows below,
 *   in one pass over the rows plus the M tail rows fetched by index.  A row with lb = -inf is not read as a number and is in no sum
 *   but, where the tail holds such rows, in the normalisation of the smoothed weights and in BFHIP_PLOO_ESS, as in bfhip_ploo_finish.
 *   With flag 1 or 4 every figure of the column but M and the flags is NaN.  work: bfhip_ploo_work_bytes(n) bytes, the two stages'.
 * n > 2^31 - 1: BFHIP_ERR_UNSUPPORTED.  Every reduction has an order fixed by n alone and a column never meets its neighbours: bitwise
 * repeatable, whichever slot or batch a column lands in.  Stream-ordered, no host synchronisation. */
#define BFHIP_LGO_NOUT 4
#define BFHIP_LGO_CHI2_BASE 0   /* sum w q, w = exp(lb) */
#define BFHIP_LGO_CHI2 1        /* sum exp(v) q under the smoothed, normalised weights */
#define BFHIP_LGO_PPP_BASE 2    /* sum w Q */
#define BFHIP_LGO_PPP 3         /* sum exp(v) Q */
int bfhip_igamc(bfhip_ctx *ctx, long n, const double *a, const double *x, double *out);
int bfhip_lgo_accum(bfhip_ctx *ctx, long n, const double *z, long ldz, int nb, const int *slot, const double *c, unsigned start,
                    double *acc, long lda);
int bfhip_lgo_finish(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, const double *c, const double *dof, const double *lb,
                     const uint64_t *tail_keys, const uint32_t *tail_idx, double *out, double *lgo_out, void *work, size_t work_bytes);

/* Marginal posterior histograms and credible levels of (weighted) draws (bayesfast_amd/utils/marginals.py has the definitions), on a
 * batch of at most BFHIP_DIAG_BATCH parameters in a (n, BFHIP_DIAG_BATCH) series buffer as bfhip_wstat_columns writes it with w = NULL.
 * Everything that is accumulated is a 64-bit integer: the weights are fixed-point numbers q, a histogram is a sum of q's, and integer
 * sums do not depend on their order -- LDS and global atomics, any launch shape, any sharding of the rows give the same bits.
 *   bfhip_marg_quantise  q[i] = floor(wp[i] 2^k) as uint64 for normalised weights wp (n,) in [0, 1] and 0 <= k <= 62 (2^k wp is exact);
 *                        wp NULL: q[i] = 1.  A weight that is negative, NaN or above 1 gets q = 0 and ADDS one to *flag (the caller
 *                        zeroes it).  With k = 62 - ceil(log2 n_all) the sum of the q of n_all draws is at most 2^62.
 *   bfhip_marg_extent    lo, hi (BFHIP_DIAG_BATCH,) <- per column the smallest and the largest FINITE value among the rows with q > 0
 *                        (q NULL: every row); +inf and -inf for a column without one.  work: BFHIP_MARG_EXTENT_WORK doubles.
 *   bfhip_marg_hist1d    for the columns b < nb and device doubles lo, hi, inv (BFHIP_DIAG_BATCH,): a finite value with lo <= x <= hi
 *                        goes to bin min(floor((x - lo) inv), n_bins - 1) -- a subtraction, then a multiplication -- anything else to
 *                        outside[b][0 .. 2]: below, above, not finite.  hist (BFHIP_DIAG_BATCH, n_bins) and outside (BFHIP_DIAG_BATCH, 3),
 *                        uint64, are ADDED to, in units of q; rows with q = 0 are not read.  1 <= n_bins <= BFHIP_MARG_MAX_BINS.
 *   bfhip_marg_index     idx[r ld + col0 + b] <- the same bin as one uint8, 255 for "not in range", b < nb, 1 <= n_bins <=
 *                        BFHIP_MARG_MAX_BINS2D; idx is a (n, ld) byte matrix, ld >= col0 + nb.
 *   bfhip_marg_hist2d    hist[p][idx[r][pairs[p][0]]][idx[r][pairs[p][1]]] += q[r] (q NULL: 1) over the rows where both indices are
 *                        below n_bins; pairs (n_pair, 2) int32 on the device (repeats and (i, i) allowed; a column outside [0, ld) adds
 *                        nothing), hist (n_pair, n_bins, n_bins) uint64, ADDED to.  idx 16-byte aligned, ld a power of two from 16 to
 *                        BFHIP_MARG_MAX_LD.  A workgroup keeps the histograms of a group of pairs in LDS as uint64 (4 pairs at 64 x 64,
 *                        one at 128 x 128 of the CU's 160 KB), reads a tile of index rows once for all of them, adds with 64-bit LDS
 *                        atomics and flushes its non-zero bins with 64-bit global atomics.
 *   bfhip_marg_levels    a workgroup per histogram of n_hist contiguous ones of m <= 16384 uint64 bins: total[h] <- S = the sum, and
 *                        levels[h n_p + i] <- the largest bin value v with (double)(sum of the bins >= v) >= probs[i] (double)S
 *                        (probs: n_p device doubles in (0, 1]); 0 for an empty histogram.  Exact: at most 64 integer counts.
 * Stream-ordered, no host synchronisation; 64-bit offsets, n <= 2^31 - 1. */
#define BFHIP_MARG_MAX_BINS 1024
#define BFHIP_MARG_MAX_BINS2D 128
#define BFHIP_MARG_MAX_LD 256
#define BFHIP_MARG_EXTENT_WORK 32768
int bfhip_marg_quantise(bfhip_ctx *ctx, long n, const double *wp, int k, uint64_t *q, uint64_t *flag);
int bfhip_marg_extent(bfhip_ctx *ctx, long n, const double *series, const uint64_t *q, double *lo, double *hi, double *work);
int bfhip_marg_hist1d(bfhip_ctx *ctx, long n, const double *series, const uint64_t *q, const double *lo, const double *hi,
                      const double *inv, int nb, int n_bins, uint64_t *hist, uint64_t *outside);
int bfhip_marg_index(bfhip_ctx *ctx, long n, const double *series, const double *lo, const double *hi, const double *inv, int nb,
                     int n_bins, uint8_t *idx, long ld, int col0);
int bfhip_marg_hist2d(bfhip_ctx *ctx, long n, const uint8_t *idx, long ld, const int32_t *pairs, long n_pair, const uint64_t *q,
                      int n_bins, uint64_t *hist);
int bfhip_marg_levels(bfhip_ctx *ctx, long n_hist, long m, const uint64_t *hist, int n_p, const double *probs, uint64_t *levels,
                      uint64_t *total);

/* The OptimizeStep's Laplace approximation (utils/laplace.py:131-183; the reference differences the gradient with numdifftools, at
 * every Newton-CG iteration and once more at the maximum, one point per call).  Both calls take the uploaded SCALAR surrogate density
 * with every feature of bfhip_density_desc; a pipeline density (bfhip_pipeline_upload) is refused with BFHIP_ERR_UNSUPPORTED
 * and has bfhip_pipeline_logp_hess / bfhip_pipeline_laplace_opt below.
 *
 * bfhip_logp_hess: Density.logp / grad and the Hessian of logp for n points: x (n,d) -> logp (n,), grad (n,d) (either may be NULL),
 * hess (n,d,d) row-major.  The Hessian is the closed form of the function bfhip_logp_grad returns -- polynomial, surrogate input
 * scaling, the linear extrapolation outside the bound, the decay term, the Gaussian link, the constraint transform when
 * original_space = 0 -- i.e. the symmetrised Jacobian of that gradient, symmetric bit for bit.  On the surfaces beta = alpha and
 * beta_d^2 = alpha_2, where the function is only C^1, it takes the branch the gradient takes.  A workgroup per point.  The output is
 * 8 n d^2 bytes; the kernel is NOT bound by those stores but by the evaluation in front of them (measured: docs/EXPERIMENTS.md).
 * Stream-ordered, no host synchronisation. */
int bfhip_logp_hess(bfhip_ctx *ctx, int n, const double *x, int original_space, double *logp, double *grad, double *hess);

typedef struct {
    int max_iter;   /* accepted steps per start */
    double xtol;    /* mean |step| <= xtol ends a start, as Newton-CG's avextol does */
} bfhip_laplace_opts;

/* n_start independent maximisations of the uploaded density in the sampling space (original_space = 0), one workgroup each, the
 * whole iteration inside one launch: Newton steps (-H + lambda I) s = g by a Cholesky factorisation in LDS, lambda = 0 tried first in
 * every iteration and raised tenfold (Levenberg) while the matrix does not factor or the step does not increase logp.
 * x0 (n_start,d) -> x (n_start,d), logp (n_start,), hess (n_start,d,d) at x (may be NULL), info (n_start,4) doubles: accepted
 * iterations; status (0 converged: mean |step| <= xtol on an UNDAMPED step, lambda = 0; 1 max_iter; 2 non-finite logp or step;
 * 3 step <= xtol but still damped, e.g. a singular Hessian); the last mean |step|; the last lambda.
 * A start's result depends on its x0 row and the density only -- not on n_start, nor on the workgroup that ran it.
 * Stream-ordered, no host synchronisation. */
int bfhip_laplace_opt(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int n_start, const double *x0, double *x, double *logp,
                      double *hess, double *info);

/* The same two calls for the PIPELINE density (bfhip_pipeline_upload: multi-output surrogate, Gaussian likelihood, optional prior), in
 * its resident forms (the sixteen- and eight-chain layouts), d <= BFHIP_MAX_DIM, with or without bound, decay term, transform, input
 * scales and prior.  The Hessian is the closed form of the function bfhip_logp_grad returns for that density
 * (csrc/bfhip_pld_hess.h has the derivation), symmetric bit for bit; on the surfaces beta = alpha and beta_d^2 = alpha_2 it takes the
 * gradient's branch.  hess_kind selects the matrix:
 *   BFHIP_HESS_FULL           H = -G^T G - sum_o r_o d2 f_o + (chain, prior, decay, transform terms), G the Jacobian of the (whitened,
 *                             extrapolated) outputs in the scaled coordinates and r their residual
 *   BFHIP_HESS_GAUSS_NEWTON   every term that carries the residual dropped: -a G^T G a, the prior's -prec_i J_i^2, the decay term and
 *                             the transform's log-Jacobian term.  Its likelihood part is negative semi-definite by construction: what
 *                             a Laplace covariance and a damped Newton step want far from the maximum.
 * bfhip_pipeline_logp_hess: x (n,d) -> logp (n,), grad (n,d) (either may be NULL), hess (n,d,d) row-major.  A workgroup per point;
 * the two dense contractions run on the FP64 matrix cores.
 * bfhip_pipeline_laplace_opt: as bfhip_laplace_opt, same iteration, same statuses, info laid out the same; hess_kind selects both
 * the matrix of the iteration and the one returned (hess may be NULL).
 * BFHIP_ERR_UNSUPPORTED: a scalar density (use the two calls above); the streamed form of the pipeline density; an LDS or work-buffer
 * need of one workgroup above the limit (the message names the numbers).  
 * Work buffer: both calls need min(n, 2 per CU) slots of (MP + DG) DG doubles in a buffer that belongs to the context, only grows, is
 * capped at 256 MB and is freed by bfhip_ctx_destroy.  A call that finds it too small SYNCHRONISES the stream and allocates: that call
 * is neither stream-ordered nor fit for graph capture.  Warm the buffer up first -- one call with the largest n that will be used,
 * for the density that will be used -- before capturing a graph or timing; every later call of at most that need is stream-ordered
 * with no host synchronisation. */
#define BFHIP_HESS_FULL 0
#define BFHIP_HESS_GAUSS_NEWTON 1
int bfhip_pipeline_logp_hess(bfhip_ctx *ctx, int n, const double *x, int original_space, int hess_kind, double *logp, double *grad,
                             double *hess);
int bfhip_pipeline_laplace_opt(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int hess_kind, int n_start, const double *x0, double *x,
                               double *logp, double *hess, double *info);

/* Profiles of the uploaded density: at every value of one coordinate, the maximum over the coordinates that are not held fixed.
 * n_line independent grid lines, one workgroup each (the pipeline form: a capped grid whose workgroups walk over the lines), every
 * array in the SAMPLING coordinates.  Line l holds the coordinates with fixed[l][i] != 0 at their x_start[l] values, except
 * walk[l], which must be one of them: for k = 0 .. n_val - 1 it sets x[walk[l]] = values[l][k], maximises the objective over the
 * free coordinates with the iteration of bfhip_laplace_opt -- from the optimum of value k - 1, from x_start[l] for k = 0; no tangent
 * predictor -- and writes the point x[l][k], the objective's value logp[l][k] and info[l][k] (the four numbers of bfhip_laplace_opt).
 * A fixed coordinate's step is exactly zero: it is returned with the bits it was given.  The convergence measure, the damping
 * scale and the Levenberg shift range over the free coordinates; a line with none evaluates once per value (status 0, 0 iterations).
 *   objective BFHIP_PROFILE_SAMPLING   the function bfhip_laplace_opt climbs (the sampling-space density)
 *             BFHIP_PROFILE_ORIGINAL   the original-space density parametrised by the sampling coordinates, logp_orig(T(x)): the
 *                                      sampling-space one without the transform's log-Jacobian, and where the decay term is on
 *                                      with that term's true derivatives (the sampling-space gradient carries it without the
 *                                      transform's Jacobian).  What a profile is taken of; hard bounds stay respected.  Without a
 *                                      transform both are the same function, bit for bit.
 *   a NaN in values ends its line: that column and the later ones hold NaN and status 4 (not run)
 *   a maximisation that ends with status 2 is written as such; the next value starts from the last optimum whose status was not 2
 *   walk[l] = -1 moves nothing: one masked maximisation from x_start[l].  It takes n_val == 1 (values may then be NULL).  With an
 *   all-zero mask and BFHIP_PROFILE_SAMPLING it returns what bfhip_laplace_opt / bfhip_pipeline_laplace_opt return, bit for bit.
 * BFHIP_ERR_ARG: an unknown objective; n_val < 1; a walk coordinate out of range or outside its line's mask; walk = -1 with n_val != 1.
 * BFHIP_ERR_UNSUPPORTED: the scalar call on a pipeline density and the reverse; the pipeline call where bfhip_pipeline_laplace_opt
 * refuses (the streamed form, an LDS or work-buffer need above the limit); it uses the same work buffer, grown the same way.
 * A line's result depends on its own rows and the density only -- not on n_line, nor on the workgroup that ran it.
 * Both calls read fixed and walk back to check them: they SYNCHRONISE the stream before they launch. */
#define BFHIP_PROFILE_SAMPLING 0
#define BFHIP_PROFILE_ORIGINAL 1
#define BFHIP_PROFILE_NOT_RUN 4
int bfhip_profile_lines(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int objective, int n_line, int n_val, const uint8_t *fixed,
                        const int32_t *walk, const double *x_start, const double *values, double *x, double *logp, double *info);
int bfhip_pipeline_profile_lines(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int hess_kind, int objective, int n_line, int n_val,
                                 const uint8_t *fixed, const int32_t *walk, const double *x_start, const double *values, double *x,
                                 double *logp, double *info);

/* The sampler kernels' sum over the 64 lanes of a wave (csrc/bfhip_wave.h: v_mfma_f64_4x4x4 steps on the matrix pipe and two row
 * rotations), on given lane values: in (n_batch, n_val, 64) -> out (n_batch, n_val), n_val values reduced together as the kernels
 * reduce them, 1 <= n_val <= BFHIP_WSUM_MAX.  form BFHIP_WSUM_BUILT is the form the library's kernels were built with,
 * BFHIP_WSUM_PACKED the second step shared by four values, BFHIP_WSUM_UNPACKED the second step once per value; all three give the
 * same bits (tests/test_gpu_wave_sum.py holds them to that and to an emulation of the instruction's lane maps).  A check of the
 * reduction on the device it runs on, not a compute path.  Stream-ordered, no host synchronisation. */
#define BFHIP_WSUM_MAX 7
#define BFHIP_WSUM_BUILT 0
#define BFHIP_WSUM_PACKED 1
#define BFHIP_WSUM_UNPACKED 2
int bfhip_wave_sum_probe(bfhip_ctx *ctx, int n_batch, int n_val, int form, const double *in, double *out);
/* The same reduction with its results left in the vector registers (csrc/bfhip_wave.h: wave_sum_packs), in the form the library was
 * built with: out (n_batch, n_val) the values read one by one (get), flag (n_batch) ints, 1 where any_le0() holds -- some value of
 * the batch is <= 0., an ordered compare: false for NaN, true for +-0. and -inf -- which the U-turn tests of the NUTS kernels take
 * without reading a sum.  Same argument rules. */
int bfhip_wave_packs_probe(bfhip_ctx *ctx, int n_batch, int n_val, const double *in, double *out, int *flag);

/* NOT part of this interface: the library's test and tuning switches (force a chain layout, a kernel form or a chains-per-workgroup
 * count; attach measurement buffers; run a launch in one part).  They have ONE entry point each for integers and for buffers,
 * declared with their keys in include/bfhip_debug.h; they never change what a call computes, and a binding has no use for them. */

#ifdef __cplusplus
}
#endif
#endif
