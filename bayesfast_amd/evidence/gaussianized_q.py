"""Gaussianized importance sampling and Gaussianized harmonic mean (reference: bayesfast/evidence/gaussianized.py:219-286): the
evidence of a posterior from its samples through a ``SIT`` density q fitted to them.  GIS fits q on all the samples and feeds
fresh draws from q to ``importance``; GHM fits q on the first half and evaluates ``harmonic`` on the second half.

Both take GBS's device-resident route (evidence/gbs.py) when the samples are a one-rank ``TraceTuple`` of device tensors: the
samples, halves, draws and log-densities then stay on the GPU, and ``importance`` / ``harmonic`` reduce them there."""
import warnings

import numpy as np

from .gbs import (_WRONG_LOGP_P, _checked_shape, _checked_sit, _device_density, _device_samples, _draws_from_q, _evaluate,
                  _host_samples, _optional_positive)
from .harmonic import harmonic
from .importance import importance

__all__ = ['GIS', 'GHM']


class GIS:
    """``GIS(sit=None, parallel_backend=None, n_q=None, f_call=0.05)``: the arguments and their rules are GBS's (``n_q`` draws
    from the fitted SIT, or ``f_call`` times the density calls of a ``TraceTuple``); ``parallel_backend`` is accepted and
    ignored."""

    def __init__(self, sit=None, parallel_backend=None, n_q=None, f_call=0.05):
        self.sit = _checked_sit(sit)
        self.n_q = _optional_positive(n_q, int, 'n_q')
        self.f_call = _optional_positive(f_call, float, 'f_call')

    def run(self, x_p, logp, logp_p=None):
        """x_p: posterior samples (n, d), (chain, iteration, d) or a ``TraceTuple``; logp: the unnormalised log-posterior;
        logp_p: accepted and ignored, as in the reference.  Returns ``(logz, logz_err)``."""
        from ..utils.threads import blas_single_thread
        if not callable(logp):
            raise ValueError('logp should be callable.')
        with blas_single_thread():   # (as GBS.run)
            return self._run(x_p, logp)

    __call__ = run

    def _run(self, x_p, logp):
        from ..samplers.sample_trace import TraceTuple
        if isinstance(x_p, TraceTuple):
            dev = self._run_on_device(x_p, logp)
            if dev is not None:
                return dev
        n_call, x_p = _host_samples(x_p)
        n_samples, x_p = _checked_shape(x_p)
        n_q = _draws_from_q(self.n_q, self.f_call, n_samples, n_call)
        self.sit.fit(data=x_p)
        x_q = self.sit.sample(n_q)[0]
        return importance(_evaluate(logp, x_q), self.sit.logq(x_q))

    def _run_on_device(self, trace, logp):
        """The samples where ``sample()`` left them, the default Sobol generator and ``logp`` a ``SurrogateDensity``'s: the fit,
        the draws and both log-densities on the GPU; only the three scalars of the reduction reach the host.  None when any
        of that does not hold (the host route runs)."""
        from ..utils import sobol
        den = _device_density(logp)
        if den is None or self.sit.mvn_generator is not sobol.multivariate_normal:
            return None
        x_p = _device_samples(trace)
        if x_p is None:
            return None
        n_samples, x_p = _checked_shape(x_p)
        n_q = _draws_from_q(self.n_q, self.f_call, n_samples, trace.n_call)
        self.sit.fit(data=x_p.reshape(-1, x_p.shape[-1]))
        x_q = self.sit._sample_device(n_q)
        return importance(den.device().logp_and_grad(x_q, True)[0], self.sit._logq_device(x_q))


class GHM:
    """``GHM(sit=None, parallel_backend=None)``: ``sit`` a ``SIT``, the keyword arguments of one, or None; ``parallel_backend``
    is accepted and ignored."""

    def __init__(self, sit=None, parallel_backend=None):
        self.sit = _checked_sit(sit)

    def run(self, x_p, logp=None, logp_p=None):
        """x_p: posterior samples (n, d), (chain, iteration, d) or a ``TraceTuple``; logp: the unnormalised log-posterior, needed
        unless logp_p, its values on x_p, is given with the shape of x_p's samples.  Returns ``(logz, logz_err)``."""
        from ..utils.threads import blas_single_thread
        with blas_single_thread():   # (as GBS.run)
            return self._run(x_p, logp, logp_p)

    __call__ = run

    def _run(self, x_p, logp, logp_p):
        from ..samplers.sample_trace import TraceTuple
        if isinstance(x_p, TraceTuple):
            dev = self._run_on_device(x_p, logp, logp_p)
            if dev is not None:
                return dev
        _, x_p = _host_samples(x_p)
        _, x_p = _checked_shape(x_p)
        cut = x_p.shape[0] // 2
        known = self._known_logp_p(logp_p, x_p.shape[:-1], cut, callable(logp))
        if known is None:
            known = _evaluate(logp, x_p[cut:])
        self.sit.fit(data=x_p[:cut])
        return harmonic(known, self.sit.logq(x_p[cut:]))

    @staticmethod
    def _known_logp_p(logp_p, lead, cut, can_compute):
        """logp_p's second half when its shape is ``lead``; None (with the reference's warning) when it is not, and the
        reference's error when logp cannot stand in for it."""
        import torch
        known = None
        if logp_p is not None:
            known = logp_p if isinstance(logp_p, torch.Tensor) and logp_p.is_cuda else np.asarray(logp_p)
            if tuple(known.shape) == tuple(lead):
                known = known[cut:]
            else:
                warnings.warn(_WRONG_LOGP_P, RuntimeWarning)
                known = None
        if known is None and not can_compute:
            raise ValueError('you gave me neither the correct logp_p nor a callable logp function.')
        return known

    def _run_on_device(self, trace, logp, logp_p):
        """The samples where ``sample()`` left them and either a ``SurrogateDensity``'s ``logp`` or a logp_p of the right shape: the
        halves, the fit and both log-densities on the GPU; the normalised terms visit the host for the autocorrelation time.
        GHM draws nothing from q, so the SIT's generator does not matter.  None when that does not hold (the host route runs)."""
        den = _device_density(logp)
        x_p = _device_samples(trace)
        if x_p is None:
            return None
        _, x_p = _checked_shape(x_p)
        lead = tuple(x_p.shape[:-1])
        fits = logp_p is not None and tuple(np.shape(logp_p)) == lead
        if den is None and not fits:
            return None
        cut = lead[0] // 2
        d = x_p.shape[-1]
        test = x_p[cut:].reshape(-1, d).contiguous()
        test_lead = (lead[0] - cut,) + lead[1:]
        known = self._known_logp_p(logp_p, lead, cut, True)
        if known is None:
            known = den.device().logp_and_grad(test, True)[0].reshape(test_lead)
        self.sit.fit(data=x_p[:cut].reshape(-1, d))
        return harmonic(known, self.sit._logq_device(test).reshape(test_lead))
