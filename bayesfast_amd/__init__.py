"""bayesfast_amd: MI355X-native implementation of BayesFast's data-parallel hot path.

Polynomial-surrogate logp/grad, leapfrog, NUTS/HMC over many chains and the surrogate's least-squares fit
run as hand-written gfx950 HIP kernels behind a C ABI (include/bfhip.h); this package is the thin Python
host side that mirrors the reference's ``modules`` / ``samplers`` / ``core.sample`` interfaces for that path.
"""
from . import _lib  # noqa: F401
from .modules import PolyConfig, PolyModel, FitReport, RidgeReport
from .core.module import Surrogate
from .core.density import SurrogateDensity, Chi2PipelineDensity, GaussianLink
from .core.sample import sample
from .samplers import NTrace, HTrace, TNTrace, GaussianBase, TraceTuple
from .utils import SystematicResampler, data_loo, pointwise_loo, DataLOO, reweight_moments, data_reweight, Reweighted
from .utils import data_lgo, grouped_loo, group_whitening_of, DataLGO
from .utils import power_scale, data_power_scale, PowerScale
from .core.refit import select_fit_points, importance_weights
from .transforms import SIT
from .evidence import GBS, GIS, GHM, bridge, importance, harmonic

__all__ = ['PolyConfig', 'PolyModel', 'FitReport', 'RidgeReport', 'Surrogate', 'SurrogateDensity', 'Chi2PipelineDensity', 'GaussianLink', 'sample', 'NTrace', 'HTrace', 'TNTrace', 'GaussianBase', 'TraceTuple',
           'SystematicResampler', 'select_fit_points', 'importance_weights', 'SIT', 'GBS', 'GIS', 'GHM', 'bridge', 'importance',
           'harmonic', 'data_loo', 'pointwise_loo', 'DataLOO', 'reweight_moments', 'data_reweight', 'Reweighted',
           'data_lgo', 'grouped_loo', 'group_whitening_of', 'DataLGO', 'power_scale', 'data_power_scale', 'PowerScale']
