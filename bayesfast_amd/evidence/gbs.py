"""Gaussianized bridge sampling (reference: bayesfast/evidence/gaussianized.py:179-216): the evidence of a posterior from
its samples.  The first half of the samples trains a ``SIT`` density q, the second half and fresh draws from q feed the
bridge estimator, and since q is normalised the bridge's log r is the log-evidence."""
import warnings

import numpy as np

from ..transforms.sit import SIT
from .bridge import bridge

__all__ = ['GBS']


def _optional_positive(value, kind, name):
    if value is None:
        return None
    try:
        value = kind(value)
    except Exception:
        value = None
    if value is None or not value > 0:
        raise ValueError('invalid value for {}.'.format(name))
    return value


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
    return t[:, trace._start():]


def _device_density(logp):
    """The ``SurrogateDensity`` whose ``logp`` (or itself) ``logp`` is, or None."""
    from ..core.density import SurrogateDensity
    if type(logp) is SurrogateDensity:
        return logp
    den = getattr(logp, '__self__', None)
    if isinstance(den, SurrogateDensity) and getattr(logp, '__func__', None) in (SurrogateDensity.logp, SurrogateDensity.__call__):
        return den
    return None


def _evaluate(logp, points):
    """logp on an array of points (..., d): in one call when the callable takes a batch, point by point otherwise."""
    lead, d = points.shape[:-1], points.shape[-1]
    rows = points.reshape(-1, d)
    values = None
    try:
        values = np.asarray(logp(rows), dtype=np.float64)
        if values.shape != (rows.shape[0],):
            values = None
    except Exception:
        values = None
    if values is None:
        values = np.array([logp(row) for row in rows], dtype=np.float64)
    return values.reshape(lead)


def _draws_from_q(n_q, f_call, n_samples, n_call):
    """How many draws to take from the fitted SIT: ``n_q`` if given, else ``f_call`` times the sampler's density calls (known for
    a ``TraceTuple`` only), else as many as there are samples."""
    if n_q is not None:
        return n_q
    if f_call is not None:
        if n_call is not None:
            return int(n_call * f_call)
        warnings.warn('f_call should be used only when x_p is a TraceTuple. Using equal-sample allocation for now.',
                      RuntimeWarning)
    return n_samples


class GBS:
    """``GBS(sit=None, parallel_backend=None, n_q=None, f_call=0.05)`` with the reference's meaning: ``sit`` a ``SIT``, the
    keyword arguments of one, or None; ``n_q`` draws from the fitted SIT, or ``f_call`` times the number of density calls
    the sampler spent when the samples come as a ``TraceTuple``.  ``parallel_backend`` is accepted and ignored."""

    def __init__(self, sit=None, parallel_backend=None, n_q=None, f_call=0.05):
        self.sit = _checked_sit(sit)
        self.n_q = _optional_positive(n_q, int, 'n_q')
        self.f_call = _optional_positive(f_call, float, 'f_call')

    def run(self, x_p, logp, logp_p=None):
        """x_p: posterior samples (n, d), (chain, iteration, d) or a ``TraceTuple``; logp: the unnormalised log-posterior;
        logp_p: its values on x_p if already known.  Returns ``(logz, logz_err)``."""
        from ..utils.threads import blas_single_thread
        if not callable(logp):
            raise ValueError('logp should be callable.')
        # (host BLAS on one thread, as the reference runs it, core/sample.py:167: the d x d factorisations of a SIT fit gain nothing
        # from threads, and OpenBLAS workers spinning after each call exhaust a container's CPU quota -- every thread of the process,
        # the ROCm runtime's included, then stands still until the next 100 ms scheduling period: nine such stalls were 0.5 s of a
        # config-5 GBS run)
        with blas_single_thread():
            return self._run(x_p, logp, logp_p)

    def _run(self, x_p, logp, logp_p):
        from ..samplers.sample_trace import TraceTuple
        if isinstance(x_p, TraceTuple):
            dev = self._run_on_device(x_p, logp, logp_p)
            if dev is not None:
                return dev
        n_call, x_p = _host_samples(x_p)
        n_samples, x_p = _checked_shape(x_p)
        n_q = _draws_from_q(self.n_q, self.f_call, n_samples, n_call)
        cut = x_p.shape[0] // 2
        train, test = x_p[:cut], x_p[cut:]
        self.sit.fit(data=train)
        x_q = self.sit.sample(n_q)[0]
        known = None
        if logp_p is not None:
            known = np.asarray(logp_p)
            if known.shape == x_p.shape[:-1]:
                known = known[cut:]
            else:
                warnings.warn(_WRONG_LOGP_P, RuntimeWarning)
                known = None
        if known is None:
            known = _evaluate(logp, test)
        return bridge(known, _evaluate(logp, x_q), self.sit.logq(test), self.sit.logq(x_q))

    def _run_on_device(self, trace, logp, logp_p):
        """The same estimate with the samples where ``sample()`` left them: a TraceTuple of one rank whose arrays are device tensors,
        a SIT with the default generator and ``logp`` the ``logp`` method of a ``SurrogateDensity`` (whose kernel takes device
        tensors).  The halves, the SIT's draws and the four log-density vectors stay on the GPU; only the vectors (n,) visit the
        host, for ``bridge``.  None when any of that does not hold (the host path runs)."""
        from ..utils import sobol
        den = _device_density(logp)
        if den is None or self.sit.mvn_generator is not sobol.multivariate_normal:
            return None
        x_p = _device_samples(trace)   # (None for more than one rank, or a trace without a device tensor)
        if x_p is None:
            return None
        n_samples, x_p = _checked_shape(x_p)
        n_q = _draws_from_q(self.n_q, self.f_call, n_samples, trace.n_call)
        cut = x_p.shape[0] // 2
        d = x_p.shape[-1]
        train, test = x_p[:cut].reshape(-1, d), x_p[cut:].reshape(-1, d).contiguous()
        self.sit.fit(data=train)
        x_q = self.sit._sample_device(n_q)
        dd = den.device()
        known = None
        if logp_p is not None:
            known = np.asarray(logp_p)
            if known.shape == tuple(x_p.shape[:-1]):
                known = known[cut:]
            else:
                warnings.warn(_WRONG_LOGP_P, RuntimeWarning)
                known = None
        if known is None:
            known = dd.logp_and_grad(test, True)[0].cpu().numpy().reshape(tuple(x_p.shape[:-1])[0] - cut, *x_p.shape[1:-1])
        logp_q = dd.logp_and_grad(x_q, True)[0].cpu().numpy()
        logq_p = self.sit._logq_device(test).cpu().numpy().reshape(np.shape(known))
        return bridge(known, logp_q, logq_p, self.sit._logq_device(x_q).cpu().numpy())

    __call__ = run
