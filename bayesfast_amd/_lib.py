"""ctypes binding of libbfhip.so (include/bfhip.h).  The HIP extension is mandatory: there is no CPU
fallback, and every compute entry point fails loudly when the library is missing."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# BFHIP_LIBRARY overrides the in-tree library (tuning builds of tools/gvariant.sh)
LIB_PATH = os.environ.get('BFHIP_LIBRARY') or os.path.join(_HERE, 'libbfhip.so')
CSRC = os.path.join(_HERE, 'csrc')

SC_FIELDS = ('log_step', 'log_bar', 'hbar', 'mu', 'count', 'fg_n', 'bg_n', 'n_samples', 'prev_update',
             'adapt_window', 'i_iter', 'error')
SC_N = len(SC_FIELDS)
VEC_FIELDS = ('q', 'var', 'fg_mean', 'fg_raw', 'bg_mean', 'bg_raw')
VEC_N = len(VEC_FIELDS)
MAT_N = 6  # BFHIP_MAT_N: per-chain matrices of the full-rank metric (slot 0 = covariance)
STAT_STRIDE = 11
NSTATS = ('logp', 'energy', 'tree_depth', 'tree_size', 'mean_tree_accept', 'step_size', 'step_size_bar',
          'warmup', 'energy_change', 'max_energy_change', 'diverging')
HSTATS = ('logp', 'energy', 'n_int_step', 'accept_stat', 'accepted', 'step_size', 'step_size_bar', 'warmup',
          'energy_change', 'diverging')
MAX_DIM = 128
MAX_TREEDEPTH = 12
TREE_MODE_WORK = 4162   # BFHIP_TREE_MODE_WORK
# lower edges of the size classes of bfhip_tree_size_mode_share (bf_lag_edge): 1, 2, 3, 4, 6, 8, 12, 16, ...
LAG_EDGES = tuple((j + 1) if j < 2 else ((1 << ((j + 1) // 2)) if (j & 1) else (3 << (j // 2 - 1))) for j in range(64))

_dp = C.POINTER(C.c_double)
_u8p = C.POINTER(C.c_uint8)


class DensityDesc(C.Structure):
    _fields_ = [('d', C.c_int), ('ranges', _dp), ('hard_bounds', _u8p), ('su_lo', _dp), ('su_diff', _dp),
                ('c0', C.c_double), ('lin', _dp), ('quad', _dp), ('cubic2', _dp), ('cubic3', _dp),
                ('use_bound', C.c_int), ('mu', _dp), ('hess', _dp), ('alpha', C.c_double), ('f_mu', C.c_double),
                ('use_decay', C.c_int), ('decay_mu', _dp), ('decay_hess', _dp), ('decay_alpha2', C.c_double),
                ('decay_gamma', C.c_double),
                ('link_kind', C.c_int), ('link_y', C.c_double), ('link_prec', C.c_double), ('link_logp0', C.c_double)]


class SamplerConfig(C.Structure):
    _fields_ = [('sampler', C.c_int), ('n_warmup', C.c_int), ('max_treedepth', C.c_int), ('n_int_step', C.c_int),
                ('max_change', C.c_double), ('target_accept', C.c_double), ('gamma', C.c_double), ('k', C.c_double),
                ('t_0', C.c_double), ('adapt_step_size', C.c_int), ('adapt_metric', C.c_int),
                ('update_window', C.c_int), ('doubling', C.c_int), ('full_metric', C.c_int), ('metric_mat', C.c_void_p),
                ('chain_layout', C.c_int)]


class Tempering(C.Structure):  # bfhip_tempering
    _fields_ = [('base_S', C.c_void_p), ('base_lin', C.c_void_p), ('base_c0', C.c_double), ('logxi', C.c_double)]


class PolymodelDesc(C.Structure):  # bfhip_polymodel_desc
    _fields_ = [('d', C.c_int), ('m', C.c_int), ('c0', C.POINTER(C.c_double)), ('lin', C.POINTER(C.c_double)),
                ('quad', C.POINTER(C.c_double)), ('use_bound', C.c_int), ('mu', C.POINTER(C.c_double)),
                ('hess', C.POINTER(C.c_double)), ('alpha', C.c_double), ('f_mu', C.POINTER(C.c_double)),
                ('n2', C.c_int), ('mask2', C.POINTER(C.c_int)), ('cubic2', C.POINTER(C.c_double)),
                ('n3', C.c_int), ('mask3', C.POINTER(C.c_int)), ('cubic3', C.POINTER(C.c_double))]


class PipelineDesc(C.Structure):  # bfhip_pipeline_desc
    _fields_ = [('d', C.c_int), ('m', C.c_int), ('ranges', _dp), ('hard_bounds', _u8p), ('su_lo', _dp), ('su_diff', _dp),
                ('model', PolymodelDesc), ('y', _dp), ('prec', _dp), ('prec_diag', _dp), ('logp0', C.c_double),
                ('prior_mu', _dp), ('prior_prec', _dp), ('prior_c0', C.c_double),
                ('use_decay', C.c_int), ('decay_mu', _dp), ('decay_hess', _dp), ('decay_alpha2', C.c_double),
                ('decay_gamma', C.c_double)]


class LaplaceOpts(C.Structure):  # bfhip_laplace_opts
    _fields_ = [('max_iter', C.c_int), ('xtol', C.c_double)]


# every symbol include/bfhip.h declares: (restype, argtypes)
_vp = C.c_void_p
SYMBOLS = {
    'bfhip_version': (C.c_int, []),
    'bfhip_last_error': (C.c_char_p, []),
    'bfhip_ctx_create': (C.c_int, [C.POINTER(_vp), C.c_int, _vp]),
    'bfhip_ctx_destroy': (None, [_vp]),
    'bfhip_ctx_set_stream': (C.c_int, [_vp, _vp]),
    'bfhip_ctx_synchronize': (C.c_int, [_vp]),
    'bfhip_density_upload': (C.c_int, [_vp, C.POINTER(DensityDesc)]),
    'bfhip_logp_grad': (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, _vp]),
    'bfhip_constraint': (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    'bfhip_leapfrog': (C.c_int, [_vp, C.c_int] + [_vp] * 8),
    'bfhip_sampler_run': (C.c_int, [_vp, C.POINTER(SamplerConfig), C.c_int, C.c_int, _vp, _vp, _vp, C.c_int,
                                    C.c_int, _vp, _vp, _vp]),
    'bfhip_tnuts_run': (C.c_int, [_vp, C.POINTER(SamplerConfig), C.POINTER(Tempering), C.c_int, C.c_int, _vp, _vp, _vp, _vp,
                                  C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    'bfhip_rng_seed': (C.c_int, [_vp, C.c_int, C.c_uint64, C.c_uint64, _vp]),
    'bfhip_chain_init': (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, _vp, C.c_double, C.c_int, _vp, _vp]),
    'bfhip_metric_init_full': (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_double, _vp, _vp]),
    'bfhip_polymodel_upload': (C.c_int, [_vp, C.POINTER(PolymodelDesc)]),
    'bfhip_polymodel_eval': (C.c_int, [_vp, C.c_int, _vp, _vp, _vp]),
    'bfhip_polymodel_columns': (C.c_int, [_vp, C.c_int, C.c_long, C.c_long, C.c_long, _vp, C.c_int, C.c_long, _vp, _vp, C.c_int, C.c_int,
                                          _vp, C.c_long, _vp]),
    'bfhip_chi2_stage': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, C.c_double, _vp, _vp]),
    'bfhip_pipeline_upload': (C.c_int, [_vp, C.POINTER(PipelineDesc)]),
    'bfhip_design_block': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int]),
    'bfhip_gram': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    'bfhip_tree_size_mode_share': (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_double, _vp]),
    'bfhip_solve_spd': (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    'bfhip_lstsq': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp]),
    'bfhip_lstsq_loo': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  C.c_size_t]),
    'bfhip_ridge_path': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_long,
                                   _vp, _vp, _vp, _vp, _vp, C.c_size_t]),
    'bfhip_ridge_rotate': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp, C.c_int]),
    'bfhip_sort_keys': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp]),
    'bfhip_order_keys': (C.c_int, [_vp, C.c_long, _vp, _vp]),
    'bfhip_count_keys': (C.c_int, [_vp, C.c_long, _vp, C.c_long, _vp, C.c_int, _vp]),
    'bfhip_importance_weights': (C.c_int, [_vp, C.c_long, _vp, _vp, C.c_double, _vp, _vp]),
    'bfhip_polar_ns': (C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp]),
    'bfhip_ndtri': (C.c_int, [_vp, C.c_long, _vp, _vp]),
    'bfhip_ica_tanh': (C.c_int, [_vp, C.c_long, C.c_long, C.c_int, _vp, _vp]),
    'bfhip_ica_assemble': (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_long, C.c_long, _vp, _vp, _vp, _vp]),
    'bfhip_ica_post': (C.c_int, [_vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    'bfhip_spline_build': (C.c_int, [_vp, C.c_int, C.c_long, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int, _vp, C.c_double,
                                     C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    'bfhip_kde_cdf': (C.c_int, [_vp, C.c_int, C.c_long, _vp, _vp, _vp, C.c_int, _vp, _vp]),
    'bfhip_kde_work_bytes': (C.c_size_t, [C.c_long, C.c_long, C.c_int]),
    'bfhip_kde_logsum': (C.c_int, [_vp, C.c_int, C.c_long, _vp, C.c_long, _vp, C.c_long, _vp, C.c_long, C.c_int, _vp, _vp, C.c_size_t]),
    'bfhip_kde_wmean_work_bytes': (C.c_size_t, [C.c_long, C.c_long, C.c_int, C.c_int]),
    'bfhip_kde_wmean': (C.c_int, [_vp, C.c_int, C.c_long, _vp, C.c_long, _vp, C.c_int, _vp, C.c_long, C.c_long, _vp, C.c_long, C.c_int, _vp, _vp,
                                  C.c_long, _vp, C.c_size_t]),
    'bfhip_gmm_work_bytes': (C.c_size_t, [C.c_long, C.c_int, C.c_int]),
    'bfhip_gmm_step': (C.c_int, [_vp, C.c_int, C.c_int, C.c_long, _vp, C.c_long, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_long, _vp,
                                 C.c_size_t]),
    'bfhip_spline_apply': (C.c_int, [_vp, C.c_int, C.c_long, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bfhip_bridge_sums': (C.c_int, [_vp, C.c_long, _vp, C.c_long, _vp, C.c_double, _vp]),
    'bfhip_bridge_terms': (C.c_int, [_vp, C.c_long, _vp, _vp, C.c_long, _vp, _vp, C.c_double, _vp, _vp]),
    'bfhip_logmeanexp_stats': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp]),
    'bfhip_acor_moments': (C.c_int, [_vp, C.c_int, C.c_long, C.c_int, C.c_long, _vp, _vp, _vp]),
    'bfhip_acor_lag_sums': (C.c_int, [_vp, C.c_int, C.c_long, C.c_int, C.c_long, _vp, _vp, _vp, C.c_long, C.c_int, _vp, _vp]),
    'bfhip_health_chains': (C.c_int, [_vp, C.c_int, C.c_long, C.c_long, _vp, C.c_int, C.c_int, _vp, _vp]),
    'bfhip_diag_columns': (C.c_int, [_vp, C.c_int, C.c_long, C.c_long, C.c_long, _vp, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, _vp,
                                     _vp]),
    'bfhip_diag_extent': (C.c_int, [_vp, C.c_int, C.c_long, _vp, _vp, _vp]),
    'bfhip_diag_sort': (C.c_int, [_vp, C.c_long, _vp, C.c_int, _vp, _vp]),
    'bfhip_diag_rank': (C.c_int, [_vp, C.c_long, _vp, _vp, C.c_int, _vp]),
    'bfhip_psis': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp, C.c_size_t]),
    'bfhip_wstat_columns': (C.c_int, [_vp, C.c_int, C.c_long, C.c_long, C.c_long, _vp, C.c_int, C.c_long, C.c_int, C.c_int, _vp, _vp]),
    'bfhip_wstat_moments': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp]),
    'bfhip_wstat_cumweights': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp]),
    'bfhip_wstat_quantiles': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp, C.c_int, _vp]),
    'bfhip_ploo_work_bytes': (C.c_size_t, [C.c_long]),
    'bfhip_ploo_moments': (C.c_int, [_vp, C.c_long, _vp, C.c_long, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_size_t]),
    'bfhip_ploo_tail': (C.c_int, [_vp, C.c_long, _vp, C.c_long, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t]),
    'bfhip_ploo_finish': (C.c_int, [_vp, C.c_long, _vp, C.c_long, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t]),
    'bfhip_rw_work_bytes': (C.c_size_t, [C.c_long, C.c_int]),
    'bfhip_rw_finish': (C.c_int, [_vp, C.c_long, _vp, C.c_long, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_long,
                                  C.c_long, C.c_long, _vp, C.c_int, C.c_long, C.c_int, _vp, _vp, _vp, C.c_size_t]),
    'bfhip_rw_weights': (C.c_int, [_vp, C.c_long, _vp, C.c_long, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, C.c_long, _vp]),
    'bfhip_pscale_cjs': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp, C.c_long, C.c_int, _vp, _vp]),
    'bfhip_igamc': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp]),
    'bfhip_lgo_accum': (C.c_int, [_vp, C.c_long, _vp, C.c_long, C.c_int, C.POINTER(C.c_int), _dp, C.c_uint, _vp, C.c_long]),
    'bfhip_lgo_finish': (C.c_int, [_vp, C.c_long, _vp, C.c_long, C.c_int, _dp, _dp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t]),
    'bfhip_marg_quantise':(C.c_int, [_vp, C.c_long, _vp, C.c_int, _vp, _vp]),
    'bfhip_marg_extent': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp]),
    'bfhip_marg_hist1d': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, _vp]),
    'bfhip_marg_index': (C.c_int, [_vp, C.c_long, _vp, _vp, _vp, _vp, C.c_int, C.c_int, _vp, C.c_long, C.c_int]),
    'bfhip_marg_hist2d': (C.c_int, [_vp, C.c_long, _vp, C.c_long, _vp, C.c_long, _vp, C.c_int, _vp]),
    'bfhip_marg_levels': (C.c_int, [_vp, C.c_long, C.c_long, _vp, C.c_int, _vp, _vp, _vp]),
    'bfhip_logp_hess': (C.c_int, [_vp, C.c_int, _vp, C.c_int, _vp, _vp, _vp]),
    'bfhip_laplace_opt': (C.c_int, [_vp, C.POINTER(LaplaceOpts), C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'bfhip_pipeline_logp_hess': (C.c_int, [_vp, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp]),
    'bfhip_pipeline_laplace_opt': (C.c_int, [_vp, C.POINTER(LaplaceOpts), C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp]),
    'bfhip_profile_lines': (C.c_int, [_vp, C.POINTER(LaplaceOpts), C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'bfhip_pipeline_profile_lines': (C.c_int, [_vp, C.POINTER(LaplaceOpts), C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp]),
    'bfhip_wave_sum_probe': (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    'bfhip_wave_packs_probe': (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp]),
}
HESS_FULL, HESS_GAUSS_NEWTON = 0, 1   # BFHIP_HESS_FULL / _GAUSS_NEWTON: hess_kind of the bfhip_pipeline_* Hessian calls
PROFILE_SAMPLING, PROFILE_ORIGINAL, PROFILE_NOT_RUN = 0, 1, 4   # BFHIP_PROFILE_*: the objective of the profile calls; the status of a grid value that was not run
WSUM_MAX = 7            # BFHIP_WSUM_MAX: values bfhip_wave_sum_probe reduces together
WSUM_FORMS = {'built': 0, 'packed': 1, 'unpacked': 2}   # BFHIP_WSUM_BUILT / _PACKED / _UNPACKED
ACOR_MAX_GROUPS = 256   # walker groups of bfhip_acor_lag_sums: its work buffer is min(n_w, 256) * n_lag * n_d doubles
HEALTH_I = ('n_divergent', 'n_max_treedepth', 'n_leapfrog', 'max_tree_size', 'n_accepted', 'n_nonfinite', 'n_moved')   # BFHIP_HEALTH_I_*; then the depth histogram
HEALTH_I_N = len(HEALTH_I) + MAX_TREEDEPTH + 1   # BFHIP_HEALTH_I_N
HEALTH_F = ('mean_accept', 'logp_mean', 'logp_var', 'energy_mean', 'energy_var', 'bfmi', 'step_size')   # BFHIP_HEALTH_F_*
HEALTH_F_N = len(HEALTH_F)   # BFHIP_HEALTH_F_N
DIAG_BATCH = 16         # BFHIP_DIAG_BATCH: parameters per batch of the bfhip_diag_* passes (the width of their series buffers)
WSTAT_WORK = 65536      # BFHIP_WSTAT_WORK: doubles of bfhip_wstat_moments' work buffer
MARG_MAX_BINS, MARG_MAX_BINS2D, MARG_MAX_LD = 1024, 128, 256   # BFHIP_MARG_MAX_BINS / _BINS2D / _LD
MARG_EXTENT_WORK = 32768   # BFHIP_MARG_EXTENT_WORK: doubles of bfhip_marg_extent's work buffer
LOO_TILE, LOO_WS_MAX, LOO_NSUM = 64, 1 << 28, 8   # BFHIP_LOO_TILE / _WS_MAX (doubles) / _NSUM
LOO_SSE, LOO_PRESS, LOO_MAX, LOO_ARGMAX, LOO_SY, LOO_SYY, LOO_NUNIT = range(7)   # BFHIP_LOO_*: the columns of bfhip_lstsq_loo's sums
RIDGE_MAX_L, RIDGE_TILE = 32, 64   # BFHIP_RIDGE_MAX_L / _TILE


def ridge_work(n, r, m, L):
    """BFHIP_RIDGE_WORK(n, r, m, L): doubles of bfhip_ridge_path's work buffer"""
    return int(r) * RIDGE_MAX_L + (int(n) + RIDGE_TILE - 1) // RIDGE_TILE * int(L) * int(m) * 7


PLOO_ELL, PLOO_Z, PLOO_NOUT = 0, 1, 16   # BFHIP_PLOO_ELL / _Z / _NOUT
PLOO_ROWS = ('lpd', 'swe', 'waic', 'elpd_loo', 'khat', 'sigma', 'n_tail', 'cut', 'ess_loo', 'pit', 'max_r', 'flags', 'sw2', 'max_b')   # BFHIP_PLOO_LPD ...
RW_ROWS = ('log_evidence_ratio', 'khat', 'sigma', 'n_tail', 'ess', 'flags', 'cut')   # BFHIP_RW_LER ...
LGO_ROWS = ('chi2_base', 'chi2_lgo', 'ppp_base', 'ppp_lgo')   # BFHIP_LGO_CHI2_BASE ...; BFHIP_LGO_NOUT rows
RW_SUMS = 8            # BFHIP_RW_SUMS: the out block's first row of sums; BFHIP_RW_NOUT(d) = RW_SUMS + 2 (1 + 2 d) rows
RWW_ROWS = ('sum', 'khat', 'flags')   # BFHIP_RWW_SUM ...; BFHIP_RWW_NOUT = 4 rows
RWW_NOUT = 4
CJS_ROWS = ('J', 'bound', 'cjs', 'ks', 'flags')   # BFHIP_CJS_J ...; BFHIP_CJS_NOUT rows
CJS_NOUT = 5
PSCALE_TILE = 2048     # BFHIP_PSCALE_TILE: sorted positions per workgroup of bfhip_pscale_cjs
WSTAT_TILE = 2048      # sorted positions per workgroup of bfhip_wstat_cumweights: its work buffer is ceil(n / 2048) doubles


def psis_work_bytes(n):
    """BFHIP_PSIS_WORK_BYTES(n)"""
    return 16 * int(n) + 32768


def pscale_work(n):
    """BFHIP_PSCALE_WORK(n): doubles of bfhip_pscale_cjs's work buffer"""
    return (int(n) + PSCALE_TILE - 1) // PSCALE_TILE * 352


_lib = None


def build(verbose=False):
    """Compile libbfhip.so for gfx950 in tree (hipcc cross-compiles without a GPU)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(['make', '-C', CSRC, '-j4'], stdout=out)
    return LIB_PATH


def lib():
    """The loaded library.  Raises RuntimeError when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                'bayesfast_amd: the HIP extension %s is missing; build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` or `make -C bayesfast_amd/csrc`. '
                'There is no CPU fallback.' % LIB_PATH)
        # PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so): it must be in the process BEFORE this library is, so that
        # the library's libamdhip64 dependency binds to the one PyTorch uses -- two HIP runtimes in one process and the second finds
        # "no ROCm-capable device" (seen when a test fixture loaded the library ahead of the first `import torch`)
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


class BfhipError(RuntimeError):
    pass


# ---- test / tuning switches (include/bfhip_debug.h): used by tests/, tools/ and bench.py's measurement legs only ----
def debug_set(key, value):
    """One of the library's integer switches by name (process-wide)."""
    f = lib().bfhip_debug_set
    f.restype, f.argtypes = C.c_int, [C.c_char_p, C.c_longlong]
    check(f(key.encode(), int(value)))


def debug_get(key):
    f = lib().bfhip_debug_get
    f.restype, f.argtypes = C.c_longlong, [C.c_char_p]
    return int(f(key.encode()))


def debug_buffer(key, tensor_or_none):
    """Attach (a device tensor) or detach (None) one of the measurement buffers."""
    f = lib().bfhip_debug_buffer
    f.restype, f.argtypes = C.c_int, [C.c_char_p, C.c_void_p]
    check(f(key.encode(), None if tensor_or_none is None else C.c_void_p(tensor_or_none.data_ptr())))


def last_kernel():
    """The kernel the last bfhip_sampler_run dispatched to."""
    f = lib().bfhip_debug_last_kernel
    f.restype = C.c_char_p
    return f().decode()


def check(rc):
    if rc != 0:
        msg = lib().bfhip_last_error().decode()
        exc = {-1: ValueError, -2: RuntimeError, -4: NotImplementedError}.get(rc, BfhipError)
        raise exc('bfhip error %d: %s' % (rc, msg))
