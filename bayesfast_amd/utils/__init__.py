from .acor import integrated_time, AutocorrError
from .resample import SystematicResampler
from .diagnostics import rhat, ess, summary
from .psis import psis, PSISResult, weighted_summary
from .marginals import marginals, Marginals
from .predictive import predictive, Predictive
from .data_loo import data_loo, pointwise_loo, DataLOO
from .reweight import reweight_moments, data_reweight, Reweighted
from .data_lgo import data_lgo, grouped_loo, group_whitening_of, DataLGO
from .laplace import Laplace, LaplaceResult, make_positive
from .profile import profile, Profile, ProfileInterval
from .kde import kde
from .shift import parameter_shift, ParameterShift
from .modes import modes, Modes
from .gmm import gmm, GaussianMixture, gmm_step
from .power_scale import power_scale, data_power_scale, PowerScale
from .health import sampler_health, sampler_health_sharded, divergent_summary, SamplerHealth, DivergentSummary

__all__ = ['SystematicResampler', 'integrated_time', 'AutocorrError', 'Laplace', 'LaplaceResult', 'make_positive', 'rhat', 'ess', 'summary',
           'psis', 'PSISResult', 'weighted_summary', 'marginals', 'Marginals', 'predictive', 'Predictive', 'data_loo',
           'pointwise_loo', 'DataLOO', 'reweight_moments', 'data_reweight', 'Reweighted', 'profile', 'Profile', 'ProfileInterval',
           'data_lgo', 'grouped_loo', 'group_whitening_of', 'DataLGO', 'kde', 'parameter_shift', 'ParameterShift', 'modes', 'Modes',
           'power_scale', 'data_power_scale', 'PowerScale', 'sampler_health', 'sampler_health_sharded', 'divergent_summary', 'SamplerHealth',
           'DivergentSummary', 'gmm', 'GaussianMixture', 'gmm_step']
