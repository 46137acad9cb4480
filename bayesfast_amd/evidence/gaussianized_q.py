"""Gaussianized importance sampling and Gaussianized harmonic mean (reference: bayesfast/evidence/gaussianized.py:219-286): the
evidence of a posterior from its samples through a ``SIT`` density q fitted to them.  GIS fits q on all the samples and feeds
fresh draws from q to ``importance``; GHM fits q on the first half and evaluates ``harmonic`` on the second half.

Both take GBS's device-resident route (evidence/gbs.py) when the samples are a one-rank ``TraceTuple`` of device tensors: the
samples, halves, draws and log-densities then stay on the GPU, and ``importance`` / ``harmonic`` reduce them there."""
import warnings

import numpy as np

from ..transforms.sit import SIT
from .gbs import _evaluate, _optional_positive
from .harmonic import harmonic
from .importance import importance

__all__ = ['GIS', 'GHM']

_WRONG_LOGP_P = 'the logp_p you gave me seems not correct. Will recompute it from logp and x_p.'


def _checked_sit(sit):
    if isinstance(sit, SIT):
        return sit
    if sit is None or isinstance(sit, dict):
        return SIT(**(sit or {}))
    raise ValueError('invalid value for sit.')


def _host_samples(x_p):
    """(n_call or None, samples as an array (n, d) or (chain, iteration, d)) from a TraceTuple or an array-like."""
    from ..samplers.sample_trace import TraceTuple
    if isinstance(x_p, TraceTuple):
        return x_p.n_call, x_p.get(flatten=False)
    try:
        x_p = np.asarray(x_p, dtype=np.float64)
    except Exception:
        x_p = None
    if x_p is None or x_p.ndim not in (2, 3):
        raise ValueError('invalid value for x_p.')
    return None, x_p


def _checked_shape(x_p):
    """The number of samples; a single chain loses its chain axis (the halves are then halves of the iterations)."""
    n_samples = int(np.prod(x_p.shape[:-1]))
    if x_p.shape[-1] < 2 or n_samples < 2:
        raise ValueError('invalid shape for x_p.')
    return n_samples, (x_p[0] if x_p.shape[0] == 1 else x_p)


def _device_samples(trace):
    """The samples of a one-rank TraceTuple after the warm-up as the device tensor (chain, iteration, d) it holds, or None."""
    import torch
    from .. import parallel
    if parallel.world()[1] > 1:
        return None
    t = trace.device('samples_original')
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        return None
    if trace.n_warmup >= trace.i_iter - 1:
        raise ValueError('since_iter is too large. Nothing to return.')
    return t[:, trace.n_warmup:]


def _device_density(logp):
    """The ``SurrogateDensity`` whose ``logp`` (or itself) ``logp`` is, or None."""
    from ..core.density import SurrogateDensity
    if type(logp) is SurrogateDensity:
        return logp
    den = getattr(logp, '__self__', None)
    if isinstance(den, SurrogateDensity) and getattr(logp, '__func__', None) in (SurrogateDensity.logp, SurrogateDensity.__call__):
        return den
    return None


class GIS:
    """``GIS(sit=None, parallel_backend=None, n_q=None, f_call=0.05)``: the arguments and their rules are GBS's (``n_q`` draws
    from the fitted SIT, or ``f_call`` times the density calls of a ``TraceTuple``); ``parallel_backend`` is accepted and
    ignored."""

    def __init__(self, sit=None, parallel_backend=None, n_q=None, f_call=0.05):
        self.sit = _checked_sit(sit)
        self.n_q = _optional_positive(n_q, int, 'n_q')
        self.f_call = _optional_positive(f_call, float, 'f_call')

    def _draws_from_q(self, n_samples, n_call):
        if self.n_q is not None:
            return self.n_q
        if self.f_call is not None:
            if n_call is not None:
                return int(n_call * self.f_call)
            warnings.warn('f_call should be used only when x_p is a TraceTuple. Using equal-sample allocation for now.',
                          RuntimeWarning)
        return n_samples

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
        n_q = self._draws_from_q(n_samples, n_call)
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
        n_q = self._draws_from_q(n_samples, trace.n_call)
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
